"""Development aid (runs here, no GPU): one line per kernel of every translation unit of the library (csrc/build.py's SOURCES) with the
sha256 of its normalised gfx950 instruction stream and the VGPR / SGPR / LDS / scratch sizes of its kernel descriptor.  Two trees whose
output is equal run the same device code, so a refactor of the kernels' surroundings or of the host code is checked by

    python tests/isa_digest.py [CSRC_DIR] > result.txt        # CSRC_DIR: another tree's csrc/ (default: this tree's)
    diff parent.txt result.txt

The compile is csrc/build.py's (same flags, per-file extras included) with -S --cuda-device-only.  Normalised means: comments, debug and
assembler directives dropped, and every mangled symbol replaced by its demangled name without the parameter list, so that renaming a
parameter type (which changes only the mangling) leaves the digest alone while any moved or changed instruction does not.  Where a
kernel stands in its translation unit is no device code either: basic-block labels lose the function's number and the lines are sorted by
kernel name, so host code that instantiates the same kernels in another order gives the same output."""
import concurrent.futures
import hashlib
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "gaussian-splatting-reflection_amd", "csrc"))
import build as B  # noqa: E402

DESC = {"vgpr": ".amdhsa_next_free_vgpr", "sgpr": ".amdhsa_next_free_sgpr", "lds": ".amdhsa_group_segment_fixed_size",
        "scratch": ".amdhsa_private_segment_fixed_size"}


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.splitlines()
    short = {}
    for n, d in zip(names, out):
        while True:                      # drop parameter lists, innermost first: f<true>(A, B (*)(C))::lds -> f<true>::lds
            e = re.sub(r"\([^()]*\)", "", d)
            if e == d:
                break
            d = e
        short[n] = re.sub(r"^void ", "", d).replace(" ", "")
    return short


def kernels(csrc, src):
    with tempfile.TemporaryDirectory() as tmp:
        path = os.path.join(tmp, "k.s")
        cmd = [B.HIPCC] + B.FLAGS + B.EXTRA_FLAGS.get(src, []) + ["-S", "--cuda-device-only", "-o", path, os.path.join(csrc, src)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit(r.stderr[-2000:])
        text = open(path).read()
    short = demangle(sorted(set(re.findall(r"\b_Z\w+", text))))
    lines = text.splitlines()
    res = []
    for m in re.finditer(r"^\s*\.amdhsa_kernel (\S+)$", text, re.M):
        name = m.group(1)
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".section"))
        body = []
        for l in lines[start + 1:end]:
            t = l.split(";")[0].strip()
            if t and not re.match(r"\.(loc|file|cfi_|ident|p2align)", t):
                t = re.sub(r"\.LBB\d+_(\d+)", r".LBB_\1", " ".join(t.split()))      # (.LBB<position of the function in the unit>_<block>)
                body.append(re.sub(r"\b_Z\w+", lambda s: short[s.group(0)], t))
        desc = text[m.end():text.index(".end_amdhsa_kernel", m.end())]
        sizes = {k: int(re.search(re.escape(d) + r" (\d+)", desc).group(1)) for k, d in DESC.items()}
        res.append((short[name], body, sizes))
    return sorted(res, key=lambda r: r[0])


def main():
    csrc = os.path.abspath(sys.argv[1]) if len(sys.argv) > 1 else B.HERE
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as ex:      # (as build.py: at most 4 hipcc jobs at a time)
        per_source = list(ex.map(lambda src: kernels(csrc, src), B.SOURCES))
    for src, found in zip(B.SOURCES, per_source):
        for name, body, sizes in found:
            print("%s %s lines=%d vgpr=%d sgpr=%d lds=%d scratch=%d sha256=%s" % (src, name, len(body), sizes["vgpr"], sizes["sgpr"], sizes["lds"], sizes["scratch"],
                                                                                hashlib.sha256("\n".join(body).encode()).hexdigest()))


if __name__ == "__main__":
    main()
