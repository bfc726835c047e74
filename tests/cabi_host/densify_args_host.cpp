// Test infrastructure: a host program (its own main, no Python, no device) over the HOST side of the densification-plan entries
// (include/gsr_hip_densify.h): the argument checks, which come before any device call, and the scratch-size arithmetic at its limits.
// Meant for a sanitizer build of the host code: compile csrc/gsr_densify.hip and csrc/gsr_common.hip (gsr_last_error) with this file,
//   hipcc --offload-arch=gfx950 -std=c++17 -Xarch_host -fsanitize=address,undefined -I include \
//       tests/cabi_host/densify_args_host.cpp gaussian-splatting-reflection_amd/csrc/gsr_densify.hip gaussian-splatting-reflection_amd/csrc/gsr_common.hip
// and run it: every call below is refused (or is a query or a documented no-op), so nothing is launched and no pointer is dereferenced.
// Prints "densify_args_host OK <calls>" and returns 0; the first surprise returns 1.
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstring>

#include "gsr_hip_densify.h"

static int calls = 0, failures = 0;
static void expect(bool ok, const char* what) {
	calls++;
	if (!ok) { failures++; fprintf(stderr, "FAILED: %s (last error: %s)\n", what, gsr_last_error()); }
}
static bool refused(int rc, const char* entry) { return rc == GSR_E_INVALID && strncmp(gsr_last_error(), entry, strlen(entry)) == 0; }

int main() {
	float* const F = (float*)0x7f0000000000;      // fake device pointers, 256-byte aligned, never touched
	int* const I = (int*)0x7f0000100000;
	void* const S = (void*)0x7f0000200000;
	uint8_t* const B = (uint8_t*)0x7f0000300000;
	const gsr_densify_plan good = {0.0002f, 0.01f, 0.03f, 0.3f, 4.5f, 9.0f, {0.f, 0.f, 0.f}, 1, 2, 2};
	const int P = 1000;
	const size_t need = gsr_densify_plan_scratch_bytes(P, 2), huge = (size_t)1 << 40;

	// the query: zero for what the entries refuse, monotonic, no wrap-around at the limits of P * (N + 1) < 2^31
	expect(need > 0 && need % 256 == 0, "query(1000, 2)");
	expect(gsr_densify_plan_scratch_bytes(-1, 2) == 0 && gsr_densify_plan_scratch_bytes(INT_MIN, 2) == 0, "query(P < 0)");
	expect(gsr_densify_plan_scratch_bytes(P, 0) == 0 && gsr_densify_plan_scratch_bytes(P, INT_MIN) == 0, "query(N < 1)");
	expect(gsr_densify_plan_scratch_bytes(1 << 30, 1) == 0 && gsr_densify_plan_scratch_bytes(INT_MAX, INT_MAX) == 0, "query(P (N + 1) >= 2^31)");
	expect(gsr_densify_plan_scratch_bytes(1, INT_MAX) == 0 && gsr_densify_plan_scratch_bytes(1, INT_MAX - 1) > 0, "query(1, N at the limit)");
	expect(gsr_densify_plan_scratch_bytes(0, INT_MAX) > 0, "query(0, INT_MAX)");
	{
		const size_t a = gsr_densify_plan_scratch_bytes((1 << 30) - 1, 1), b = gsr_densify_plan_scratch_bytes(715827882, 2);
		expect(a >= (size_t)4 * 3 * ((1u << 30) - 1) && a < (size_t)14 << 30, "query(2^30 - 1, 1)");
		expect(b >= (size_t)4 * 4 * 715827882u && b < (size_t)13 << 30, "query(715827882, 2)");
		size_t last = 0;
		bool mono = true;
		for (int p = 0; p < 70000; p += 37) {
			const size_t q = gsr_densify_plan_scratch_bytes(p, 2);
			mono = mono && q >= last && q >= (size_t)16 * p;
			last = q;
		}
		expect(mono, "query monotonic in P");
	}

	// select
#define SELECT(P_, plan_, a, b, c, d, e, s, n, cnt, par) gsr_densify_plan_select(P_, plan_, a, b, c, d, e, s, n, cnt, par, nullptr)
	const char* sel = "gsr_densify_plan_select";
	expect(refused(SELECT(-1, &good, F, F, F, F, F, S, huge, I, I), sel), "select P < 0");
	expect(refused(SELECT(P, nullptr, F, F, F, F, F, S, need, I, I), sel), "select NULL plan");
	gsr_densify_plan bad = good;
	bad.N = 0;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, huge, I, I), sel), "select N = 0");
	bad.N = INT_MAX;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, huge, I, I), sel), "select N = INT_MAX");
	expect(refused(SELECT(INT_MAX, &bad, F, F, F, F, F, S, huge, I, I), sel), "select P = N = INT_MAX");
	bad = good;
	bad.N = 1;
	expect(refused(SELECT(1 << 30, &bad, F, F, F, F, F, S, huge, I, I), sel), "select P (N + 1) = 2^31");
	bad = good;
	bad.scale_dims = 1;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, need, I, I), sel), "select scale_dims = 1");
	bad.scale_dims = 4;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, need, I, I), sel), "select scale_dims = 4");
	bad = good;
	bad.max_grad = 0.0f;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, need, I, I), sel), "select max_grad = 0");
	bad.max_grad = -1.0f;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, need, I, I), sel), "select max_grad < 0");
	bad.max_grad = NAN;
	expect(refused(SELECT(P, &bad, F, F, F, F, F, S, need, I, I), sel), "select max_grad = NaN");
	expect(refused(SELECT(P, &good, nullptr, F, F, F, F, S, need, I, I), sel), "select NULL xyz_gradient_accum");
	expect(refused(SELECT(P, &good, F, nullptr, F, F, F, S, need, I, I), sel), "select NULL denom");
	expect(refused(SELECT(P, &good, F, F, nullptr, F, F, S, need, I, I), sel), "select NULL accum_w");
	expect(refused(SELECT(P, &good, F, F, F, nullptr, F, S, need, I, I), sel), "select NULL denom_w");
	expect(refused(SELECT(P, &good, F, F, F, F, nullptr, S, need, I, I), sel), "select NULL scaling");
	expect(refused(SELECT(P, &good, F, F, F, F, F, nullptr, need, I, I), sel), "select NULL scratch");
	expect(refused(SELECT(P, &good, F, F, F, F, F, S, need, nullptr, I), sel), "select NULL counts");
	expect(refused(SELECT(0, &good, F, F, F, F, F, S, need, nullptr, I), sel), "select P = 0 with NULL counts");
	expect(refused(SELECT(P, &good, F, F, F, F, F, S, need, I, nullptr), sel), "select NULL parents");
	expect(refused(SELECT(P, &good, F, F, F, F, F, S, need - 1, I, I), sel), "select scratch one byte short");
	expect(refused(SELECT(P, &good, F, F, F, F, F, S, 0, I, I), sel), "select scratch of no bytes");
	expect(refused(SELECT(P, &good, F, F, F, F, F, (char*)S + 4, need, I, I), sel), "select misaligned scratch");

	// rows
#define ROWS(P_, plan_, s, n, x, sc, par, cx, cs, k, m0, m1, m2, cnt) gsr_densify_plan_rows(P_, plan_, s, n, x, sc, par, cx, cs, k, m0, m1, m2, cnt, nullptr)
	const char* rows = "gsr_densify_plan_rows";
	expect(refused(ROWS(-1, &good, S, huge, F, F, I, F, F, 0, I, I, I, I), rows), "rows P < 0");
	expect(refused(ROWS(P, nullptr, S, need, F, F, I, F, F, 10, I, I, I, I), rows), "rows NULL plan");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, -1, I, I, I, I), rows), "rows k < 0");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, P + 1, I, I, I, I), rows), "rows k > P");
	expect(refused(ROWS(0, &good, S, need, F, F, I, F, F, 1, I, I, I, I), rows), "rows P = 0, k = 1");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, INT_MAX, I, I, I, I), rows), "rows k = INT_MAX");
	expect(refused(ROWS(P, &good, nullptr, need, F, F, I, F, F, 10, I, I, I, I), rows), "rows NULL scratch");
	expect(refused(ROWS(P, &good, S, need - 1, F, F, I, F, F, 10, I, I, I, I), rows), "rows scratch one byte short");
	expect(refused(ROWS(P, &good, S, need, nullptr, F, I, F, F, 10, I, I, I, I), rows), "rows NULL xyz");
	expect(refused(ROWS(P, &good, S, need, F, nullptr, I, F, F, 10, I, I, I, I), rows), "rows NULL scaling");
	expect(refused(ROWS(P, &good, S, need, F, F, nullptr, F, F, 10, I, I, I, I), rows), "rows NULL parents with k > 0");
	expect(refused(ROWS(P, &good, S, need, F, F, I, nullptr, F, 10, I, I, I, I), rows), "rows NULL child_xyz with k > 0");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, nullptr, 10, I, I, I, I), rows), "rows NULL child_scaling with k > 0");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, 10, nullptr, I, I, I), rows), "rows NULL map_param");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, 10, I, nullptr, I, I), rows), "rows NULL map_moment");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, 10, I, I, nullptr, I), rows), "rows NULL child_of");
	expect(refused(ROWS(P, &good, S, need, F, F, I, F, F, 10, I, I, I, nullptr), rows), "rows NULL counts");
	bad = good;
	bad.N = INT_MAX;
	expect(refused(ROWS(P, &bad, S, huge, F, F, I, F, F, 10, I, I, I, I), rows), "rows N = INT_MAX");

	// prune_rows
	const char* prune = "gsr_prune_rows";
	const size_t need1 = gsr_densify_plan_scratch_bytes(P, 1);
	expect(need1 > 0 && need1 <= need, "query(1000, 1)");
	expect(refused(gsr_prune_rows(-1, B, S, huge, I, I, nullptr), prune), "prune P < 0");
	expect(refused(gsr_prune_rows(1 << 30, B, S, huge, I, I, nullptr), prune), "prune P = 2^30");
	expect(refused(gsr_prune_rows(INT_MAX, B, S, huge, I, I, nullptr), prune), "prune P = INT_MAX");
	expect(refused(gsr_prune_rows(P, nullptr, S, need1, I, I, nullptr), prune), "prune NULL remove");
	expect(refused(gsr_prune_rows(P, B, nullptr, need1, I, I, nullptr), prune), "prune NULL scratch");
	expect(refused(gsr_prune_rows(P, B, S, need1, nullptr, I, nullptr), prune), "prune NULL row_map");
	expect(refused(gsr_prune_rows(P, B, S, need1, I, nullptr, nullptr), prune), "prune NULL counts");
	expect(refused(gsr_prune_rows(0, B, S, need1, I, nullptr, nullptr), prune), "prune P = 0 with NULL counts");
	expect(refused(gsr_prune_rows(P, B, S, need1 - 1, I, I, nullptr), prune), "prune scratch one byte short");
	expect(refused(gsr_prune_rows(P, B, (char*)S + 8, need1, I, I, nullptr), prune), "prune misaligned scratch");

	// scatter_rows
	const char* scatter = "gsr_scatter_rows";
	gsr_gather_group groups[17];
	for (int i = 0; i < 17; i++) groups[i] = gsr_gather_group{0, (uint64_t)i * 1000, 3};
	expect(refused(gsr_scatter_rows(nullptr, F, I, 50, groups, 2, nullptr), scatter), "scatter NULL src");
	expect(refused(gsr_scatter_rows(F, nullptr, I, 50, groups, 2, nullptr), scatter), "scatter NULL dst");
	expect(refused(gsr_scatter_rows(F, F, nullptr, 50, groups, 2, nullptr), scatter), "scatter NULL slot");
	expect(refused(gsr_scatter_rows(F, F, I, 50, nullptr, 2, nullptr), scatter), "scatter NULL groups");
	expect(refused(gsr_scatter_rows(F, F, I, 50, groups, -1, nullptr), scatter), "scatter num_groups < 0");
	expect(refused(gsr_scatter_rows(F, F, I, 50, groups, 17, nullptr), scatter), "scatter num_groups > 16");
	groups[1].width = 0;
	expect(refused(gsr_scatter_rows(F, F, I, 50, groups, 2, nullptr), scatter), "scatter zero-width group");
	expect(gsr_scatter_rows(nullptr, nullptr, nullptr, 0, groups, 2, nullptr) == 0, "scatter n_rows = 0 is a no-op");
	expect(gsr_scatter_rows(F, F, I, 50, nullptr, 0, nullptr) == 0, "scatter num_groups = 0 is a no-op");

	if (failures) { fprintf(stderr, "densify_args_host: %d of %d checks failed\n", failures, calls); return 1; }
	printf("densify_args_host OK %d\n", calls);
	return 0;
}
