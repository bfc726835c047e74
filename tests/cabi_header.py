"""The headers under include/ as tests/test_cabi.py reads them: the prototypes, the descriptor structs, and ONE mapping from the C types the
headers use to the ctypes types the binding (_gsr.ABI) must give them.  A plain module, imported by the tests that need a prototype."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INCLUDE = os.path.join(ROOT, "include")
MAIN = "gsr_hip.h"
STRUCTS = {"gsr_adam_segment": "AdamSegment", "gsr_act_segment": "ActSegment", "gsr_gather_group": "GatherGroup",
           "gsr_refl_forward": "ReflForward", "gsr_densify_plan": "DensifyPlan"}         # C name -> class of _gsr
_SCALARS = (("float", ctypes.c_float), ("uint32_t", ctypes.c_uint32), ("uint64_t", ctypes.c_uint64), ("size_t", ctypes.c_size_t),
            ("int", ctypes.c_int))


def headers():
    """Every include/gsr_hip*.h, by listing the directory: a new header is tested without anyone adding it to a list."""
    return sorted(f for f in os.listdir(INCLUDE) if re.fullmatch(r"gsr_hip\w*\.h", f))


def text(header):
    return open(os.path.join(INCLUDE, header)).read()


def source(header):
    """The header without its comments."""
    return re.sub(r"/\*.*?\*/", "", text(header), flags=re.S)


def protos(header):
    """[(return type, entry, [argument texts])]; `(void)` is no argument."""
    found = re.findall(r"(int|size_t|const char\*)\s+(gsr_\w+)\s*\(([^;]*?)\)\s*;", source(header), flags=re.S)
    return [(ret, name, [] if args.strip() == "void" else [a.strip() for a in args.split(",")]) for ret, name, args in found]


def arg_names(args):
    return [re.sub(r".*[\s\*]", "", a) for a in args]


def ctype(arg):
    """The ctypes type of an argument or a struct member, from its text (`const float* cam`, `uint64_t`, `const gsr_act_segment* segments`)."""
    import _gsr
    arg = arg.strip()
    if arg.startswith("gsr_alloc_fn"):
        return _gsr.ALLOC_FN
    m = re.match(r"(?:const\s+)?(gsr_\w+)\s*\*", arg)
    if m:
        return ctypes.POINTER(getattr(_gsr, STRUCTS[m.group(1)]))
    if "*" in arg:
        return ctypes.c_char_p if re.match(r"const\s+char\s*\*", arg) else ctypes.c_void_p
    for prefix, t in _SCALARS:
        if re.match(prefix + r"\b", arg):
            return t
    raise ValueError(f"a C type tests/cabi_header.py does not know: {arg!r}")


def restype(ret):
    return {"int": ctypes.c_int, "size_t": ctypes.c_size_t, "const char*": ctypes.c_char_p}[ret]


def structs(header):
    """The C names of the `typedef struct { ... } name;` the header defines."""
    return re.findall(r"typedef struct \{[^}]*\}\s*(\w+);", source(header), flags=re.S)


def struct_fields(header, c_name):
    """[(field, ctypes type)] of a typedef'd struct: `uint64_t begin, end;` is two fields, `float mean[3];` an array."""
    body = re.search(r"typedef struct \{([^}]*)\}\s*%s;" % c_name, source(header), flags=re.S).group(1)
    fields = []
    for decl in (d.strip() for d in body.split(";")):
        if not decl:
            continue
        m = re.fullmatch(r"(.*?[\s\*])(\w+(?:\[\d+\])?(?:\s*,\s*\w+(?:\[\d+\])?)*)", decl, flags=re.S)
        base = ctype(m.group(1))
        for d in m.group(2).split(","):
            name, _, n = d.strip().partition("[")
            fields.append((name, base * int(n[:-1]) if n else base))
    return fields
