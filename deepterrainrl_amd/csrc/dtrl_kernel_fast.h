// dtrl_kernel_fast.h -- gfx950 fast path of the per-env dense linear algebra (device code only).
//
// The lane-phase reference path (dtrl_kernel.h) keeps the joint-space inertia matrix in LDS and pays one LDS round trip
// + barrier per elimination step (rocprof/s_memtime: factorisation 20 %, forward substitution 17 %, serial row-list
// construction 15 % of an env-step). Here lane i keeps ROW i of H in VGPRs (23 doubles) and the elimination uses
// v_readlane broadcasts of the pivot column, so an LDL^T factorisation is ~250 broadcast+FMA pairs with no LDS traffic
// and no barrier; triangular solves are 22 broadcast+FMA steps each. Constraint rows are compacted with wave ballots.
// The arithmetic (operation order included) is IDENTICAL to the reference path, so both produce the same bits; the
// reference kernel stays in the library (DTRL_KERNEL=ref) and tests/test_gpu_parity.py compares the two.
//
// The factorisation is H = U D U^T, eliminating the last DoF first (leaf-to-root: no fill-in, factorize() in dtrl_kernel.h); the
// kernel is instantiated per skeleton (dtrl_topo.h) and emits only the structurally non-zero updates.
// Row layout after factorize_regs(): h[k] for k > lane = U_{lane,k}; h[lane] = d_lane; h[k] for k < lane = U_{k,lane}
// (the transpose copy, so the second substitution also only needs the lane's own registers).
#pragma once
#include "dtrl_kernel.h"
#include "dtrl_topo.h"
#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__)

#if !DTRL_WAVE_SYNC
#error "dtrl_kernel_fast.h: the register-resident path is ONE wavefront per env by construction (v_readlane broadcasts, ballots, and LDS read-then-write sequences such as warm_match_fast() that rely on a wave's LDS operations completing in issue order). -DDTRL_WAVE_SYNC=0 builds the lane-phase reference path only (ADVICE r5)"
#endif

namespace dtrl {

__device__ __forceinline__ int lane_id() { return static_cast<int>(threadIdx.x); }
// lane id the optimiser cannot see through: address / index arithmetic derived from it is recomputed where it is used instead of being
// hoisted out of the 4000-instruction physics loop as a loop invariant and spilled to scratch across it
__device__ __forceinline__ int opaque_lane()
{
	int lane = static_cast<int>(threadIdx.x);
	asm volatile("" : "+v"(lane));
	return lane;
}
// a loaded value the optimiser must have in a register HERE: the load behind it can neither be sunk into a later branch nor be moved behind this point. No instruction
template <class T>
__device__ __forceinline__ void pin_loaded(T& v) { asm volatile("" : "+v"(v)); }
// every LDS read issued so far has arrived HERE: one s_waitcnt lgkmcnt(0) (gfx9 encoding: vmcnt and expcnt left at their maxima, i.e. not waited for). For loads that
// leave a nest of branches at different depths in front of a loop: still counted as pending at the loop's head, each of their uses in the loop gets a wait of its own
__device__ __forceinline__ void lds_loads_arrived() { __builtin_amdgcn_s_waitcnt(0xc07f); }
// the EXEC-window helpers below are spelled per arithmetic type (dtrl_types.h: fp64 shipped, fp32 opt-in build)
#if defined(DTRL_REAL_F32)
#define DTRL_VFMA "v_fma_f32"
#define DTRL_VMOV "v_mov_b32"
#else
#define DTRL_VFMA "v_fma_f64"
#define DTRL_VMOV "v_mov_b64"
#endif
__device__ __forceinline__ real bcast(real v, int src)   // src must be wave-uniform
{
#if defined(DTRL_REAL_F32)
	return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), src));
#else
	int lo = __builtin_amdgcn_readlane(__double2loint(v), src);
	int hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
	return __hiloint2double(hi, lo);
#endif
}

// row `lane` of the joint-space inertia matrix from the composite quantities in LDS (same formulas and operand order as
// mass_matrix()). Only the upper triangle (column >= lane) is produced: the leaf-first factorisation never reads the rest.
// The (link, ancestor) pairs are dealt round-robin to all 64 lanes, each evaluates the closed form once and parks the value in a
// packed table in LDS (the storage of the Delassus matrix, dead at that point):
//   entries of link l (DoF l + 2) at base_l = l (l + 5) / 2: [hx, hy, H(l, link 0), ..., H(l, link l)], non-ancestor slots = 0
// i.e. the slot of DoF pair (c, d), d <= c, is base_{c-2} + d: a lane assembles its row with D loads at compile-time offsets from its
// own lane id (no per-column index arithmetic, no branches: the loads pipeline). Lanes >= D copy row 0 (finite, never read).
template <int D>
__device__ __forceinline__ void mass_row(WSFast& ws, real (&h)[D])
{
	constexpr int Lk = D - 2;                                  // links of the character this kernel is instantiated for
	constexpr int kTab = Lk * (Lk + 5) / 2;
	constexpr int kFill = (kTab + 1) & ~1;                     // even count (16-byte stores)
	static_assert(kFill <= static_cast<int>(sizeof(ws.Apk) / sizeof(real)), "mass table does not fit the packed-matrix storage");
	const int d = static_cast<int>(threadIdx.x);
	const int l = d >= 2 ? d - 2 : 0;
	const bool hinge = d >= 2 && d < D;
	real* T = ws.Apk;
	{
		struct alignas(2 * sizeof(real)) real2 { real x, y; };
		real2* T2 = reinterpret_cast<real2*>(T);
		const real2 z2 = {0.0, 0.0};
#pragma unroll
		for (int e = 0; e < (kFill / 2 + kGroup - 1) / kGroup; ++e) if (d + e * kGroup < kFill / 2) T2[d + e * kGroup] = z2;
	}
	env_sync();
	if (hinge) {
		const int base = l * (l + 5) / 2;
		const real m = ws.sm[l], mx = ws.smx[l], my = ws.smy[l];
		T[base] = -(my - m * ws.py[l]);
		T[base + 1] = (mx - m * ws.px[l]);
	}
	const int n_pairs = ws.M.n_pairs;
#pragma unroll 2
	for (int e = lane_id(); e < n_pairs; e += kGroup) {
		const int pl = ws.M.pair_l[e], pk = ws.M.pair_k[e];
		const int a = ws.M.path[pl][pk];
		const real m = ws.sm[pl], mx = ws.smx[pl], my = ws.smy[pl], I = ws.sI[pl];
		const real plx = ws.px[pl], ply = ws.py[pl];
		const real pax = ws.px[a], pay = ws.py[a];
		T[pl * (pl + 5) / 2 + 2 + a] = I - ((plx + pax) * mx + (ply + pay) * my) + m * (plx * pax + ply * pay);
	}
	env_sync();
	const real M0 = ws.sm[0];
	const real* Tl = T + (d < D ? d : 0);
	h[0] = (d == 0) ? M0 : 0.0;
	h[1] = (d == 1) ? M0 : 0.0;
#pragma unroll
	for (int c = 2; c < D; ++c) h[c] = Tl[(c - 2) * (c + 3) / 2];   // base_{c-2} + lane
	env_sync();   // T is dead; the storage may be reused
}

// ---- lane-predicated updates through EXEC ----
// The elimination steps below update "the lanes below the pivot". Written as `if (lane > k) x = fma(...)` the compiler emits the FMA
// for every lane plus two v_cndmask per double (and keeps 23 lane masks alive in SGPRs that spill to VGPR lanes and come back by
// v_readlane): 5+ VALU instructions per step for one useful FMA. The frame kernel is VALU-issue-bound, while the SALU
// port is nearly idle, so these helpers narrow EXEC with three SALU instructions around the FMA instead. The lane mask is built from an
// inline constant (no SGPR pressure). EXEC is restored inside the same asm block, so the compiler never sees a changed EXEC.
// Same operation, same operands, same rounding as the predicated C++ form: the bits do not change (fast-vs-ref parity tests).
template <int B, int E, class F>
__device__ __forceinline__ void static_for(F&& f)
{
	if constexpr (B < E) { f(std::integral_constant<int, B>{}); static_for<B + 1, E>(f); }
}
template <int B, int E, class F>
__device__ __forceinline__ void static_for_down(F&& f)   // E-1, E-2, ..., B
{
	if constexpr (B < E) { f(std::integral_constant<int, E - 1>{}); static_for_down<B, E - 1>(f); }
}
// acc = fma(-a, b, acc) on lanes >= J; b is wave-uniform (SGPR pair)
template <int J>
__device__ __forceinline__ void fnma_lanes_ge(real& acc, real a, real b)
{
	unsigned long long sv, m;
	asm("s_lshl_b64 %2, -1, %5\n\ts_and_saveexec_b64 %1, %2\n\t" DTRL_VFMA " %0, -%3, %4, %0\n\ts_mov_b64 exec, %1"
	    : "+v"(acc), "=&s"(sv), "=&s"(m) : "v"(a), "s"(b), "n"(J) : "scc");
}
// acc = fma(-a, b, acc) on lanes < I
template <int I>
__device__ __forceinline__ void fnma_lanes_lt(real& acc, real a, real b)
{
	unsigned long long sv, m;
	asm("s_bfm_b64 %2, %5, 0\n\ts_and_saveexec_b64 %1, %2\n\t" DTRL_VFMA " %0, -%3, %4, %0\n\ts_mov_b64 exec, %1"
	    : "+v"(acc), "=&s"(sv), "=&s"(m) : "v"(a), "s"(b), "n"(I) : "scc");
}
// dst = src on lane K only / on lanes < I
template <int K>
__device__ __forceinline__ void mov_lane_eq(real& dst, real src)
{
	unsigned long long sv, m;
	asm("s_lshl_b64 %2, 1, %4\n\ts_and_saveexec_b64 %1, %2\n\t" DTRL_VMOV " %0, %3\n\ts_mov_b64 exec, %1"
	    : "+v"(dst), "=&s"(sv), "=&s"(m) : "v"(src), "n"(K) : "scc");
}
template <int I>
__device__ __forceinline__ void mov_lanes_lt(real& dst, real src)
{
	unsigned long long sv, m;
	asm("s_bfm_b64 %2, %4, 0\n\ts_and_saveexec_b64 %1, %2\n\t" DTRL_VMOV " %0, %3\n\ts_mov_b64 exec, %1"
	    : "+v"(dst), "=&s"(sv), "=&s"(m) : "v"(src), "n"(I) : "scc");
}
// dst = src on lanes B <= lane < E
template <int B, int E>
__device__ __forceinline__ void mov_lanes_in(real& dst, real src)
{
	static_assert(0 <= B && B < E && E <= 64 && E - B < 64, "lane window (s_bfm_b64 takes the width modulo 64)");
	unsigned long long sv, m;
	asm("s_bfm_b64 %2, %4, %5\n\ts_and_saveexec_b64 %1, %2\n\t" DTRL_VMOV " %0, %3\n\ts_mov_b64 exec, %1"
	    : "+v"(dst), "=&s"(sv), "=&s"(m) : "v"(src), "n"(E - B), "n"(B) : "scc");
}
// dst = v as exactly ONE ds_write, in source order among the stores spelled this way: the empty asm is a barrier for memory operations, so the compiler neither merges
// two of them into one two-address write nor reorders them (it sees stores of one lane to different addresses, which it may otherwise do freely). No instruction.
__device__ __forceinline__ void lds_store_ordered(real& dst, real v)
{
	dst = v;
	asm volatile("" : : : "memory");
}

// in-register H = U D U^T, last DoF first; returns 1/d_lane. Same elimination order and operations as factorize(), minus the
// updates that are structurally zero for the skeleton Topo (exact no-ops in the dense form). The transposed copy of U (needed by
// utsolve_regs) is produced with one pass through LDS (packed triangle in the Apk storage, which is dead between mass_row() and the
// Delassus build) instead of per-entry lane selects.
// Only the upper triangle (column >= lane) is live, so the per-entry predicate of the textbook form is dropped: the other lanes
// update entries nobody reads (they are overwritten by the transposed copy), the lanes that matter execute exactly the same
// operations. One predicated move per pivot keeps the diagonal.
template <class Topo>
__device__ __forceinline__ real factorize_regs(WSFast& ws, real (&h)[Topo::L + 2])
{
	constexpr int D = Topo::L + 2;
	const int lane = static_cast<int>(threadIdx.x);
	real dinv = 0;
	static_for_down<1, D>([&](auto kc) {             // k = D-1 ... 1
		constexpr int k = decltype(kc)::value;
		const real dk = bcast(h[k], k);
		const real ak = h[k];
		const real rk = fast_recip(dk);
		mov_lane_eq<k>(dinv, rk);                       // if (lane == k) dinv = rk
		const real lik = ak * rk;
		static_for_down<0, k>([&](auto jc) {
			constexpr int j = decltype(jc)::value;
			if constexpr (dof_coupled<Topo>(j, k)) h[j] = fmadd(-lik, bcast(ak, j), h[j]);
		});
		mov_lanes_lt<k>(h[k], lik);                     // if (lane < k) h[k] = lik
	});
	{ const real r0 = fast_recip(h[0]); if (lane == 0) dinv = r0; }
	// The transposed copy: column k of U (lanes < k) goes to S[k (k - 1) / 2 + lane], lane i then reads its row back from S[i (i - 1) / 2 + k], k < i.
	// Neither side carries a per-column lane predicate in the source (`if (lane < k)` / `if (lane > k)` compile to 2 x 22 loop-invariant 64-bit lane masks that
	// live in SGPR spill lanes: a save / reload / and / restore of EXEC around every single LDS access).
	// Stores: ALL 64 lanes store column k, ascending in k. Lanes >= k land on the slots of columns k + 1 ..., which are stored later, and a wave's LDS operations
	// complete in issue order (warm_match_fast() relies on the same), so every slot of the triangle ends up with its own column's value. The overflow of the last
	// column stays inside Apk (asserted below); slots outside the triangle are read by nobody (usolve_rows() reads U[k (k - 1) / 2 + i], i < k, only; the
	// Delassus build and link_cap_drop_mask() / row_cap_drop_mask() / append_pair_rows_fast() write the storage before they read it).
	// The stores go through lds_store_ordered(): each stays one ds_write in source order (two of them merged into one two-address write would leave the order
	// of their overlapping slots open).
	// Loads: unpredicated into a temporary (lanes >= D read row 0: in bounds, unused), then one move under an EXEC window from inline constants
	// (mov_lanes_in: 3 SALU + 1 VALU, no SGPR kept). The alternative, a select per column (`h[k] = (lane > k && lane < D) ? t : h[k]`), needs the lane mask per
	// column again, which is hoisted and spilled as before. Substep loop, instructions / SGPR spill reloads (tools/isa_spills.py), windows against selects:
	// fp64 dog 6713 / 114 against 6749 / 166, fp64 raptor 6208 / 77 against 6206 / 118, fp32 dog 8614 / 161 against 8656 / 218, fp32 raptor 7404 / 70 against
	// 7498 / 136. A window around the ds_read itself would save the move but hides the LDS access from the compiler's s_waitcnt insertion.
	static_assert((D - 1) * (D - 2) / 2 + kGroup - 1 < static_cast<int>(sizeof(ws.Apk) / sizeof(real)), "the unpredicated store of U's last column leaves the packed-matrix storage");
	real* S = ws.Apk;
	static_for<1, D>([&](auto kc) {
		constexpr int k = decltype(kc)::value;
		lds_store_ordered(S[k * (k - 1) / 2 + lane], h[k]);
	});
	env_sync();
	const int base = lane < D ? lane * (lane - 1) / 2 : 0;
	static_for<0, D - 1>([&](auto kc) {
		constexpr int k = decltype(kc)::value;
		const real t = S[base + k];
		mov_lanes_in<k + 1, D>(h[k], t);                // if (lane > k && lane < D) h[k] = t
	});
	env_sync();
	return dinv;
}
// z = U^-1 rhs (lane i holds component i): from the last DoF up
template <int D>
__device__ __forceinline__ real usolve_regs(const real (&h)[D], real z)
{
	static_for_down<1, D>([&](auto kc) {
		constexpr int k = decltype(kc)::value;
		const real zk = bcast(z, k);
		fnma_lanes_lt<k>(z, h[k], zk);                  // if (lane < k) z = fma(-h[k], zk, z)
	});
	return z;
}
// the first (largest) column k > i whose elimination updates entry i of a right-hand side; 0 = none (a leaf DoF: its entry is final as given)
template <class Topo>
constexpr int first_update_col(int i)
{
	for (int k = Topo::L + 1; k > i; --k) if (dof_coupled<Topo>(i, k)) return k;
	return 0;
}
// Z_r = U^-1 Z_r in place for the rows r = 0 .. R of Z (the R constraint rows and the free right-hand side), ROW PER LANE: lane r walks its own row
// (odd row stride: no bank conflicts), right-looking from the last DoF up. U(i, k) is wave-uniform, a broadcast LDS read of the packed triangle that
// factorize_regs() left in Apk, so the R + 1 substitutions together cost the structurally non-zero updates once (129 FMAs for the dog, 89 for the raptor)
// where the lane = DoF chain of usolve_regs() pays two v_readlane and an FMA per DoF and right-hand side. Entry i sees fma(-U(i, k), z_k, .) for k descending from the
// initial value, as in forward_subst_rows() of dtrl_kernel.h and usolve_regs(); the updates left out are those with a structurally zero U(i, k).
// An accumulator is read from the row just before its first update and stored when it is final, so only the frontier of the tree is live.
template <class Topo, int kAhead = 1>
__device__ __forceinline__ void usolve_rows(WSFast& ws, int R)
{
	constexpr int D = Topo::L + 2;
	const int lane = static_cast<int>(threadIdx.x);
	if (lane > R) return;
	real* z = ws.Z[lane];
	const real* U = ws.Apk;
	real acc[D], u[D * (D - 1) / 2];   // (constant indices only: registers)
	// the LDS reads column k needs: its U entries, the accumulators it opens, z_k itself when nothing updates it
	auto fetch = [&](auto kc) {
		constexpr int k = decltype(kc)::value;
		static_for<0, k>([&](auto ic) {
			constexpr int i = decltype(ic)::value;
			if constexpr (dof_coupled<Topo>(i, k)) u[k * (k - 1) / 2 + i] = U[k * (k - 1) / 2 + i];
			if constexpr (first_update_col<Topo>(i) == k) acc[i] = z[i];
		});
		if constexpr (first_update_col<Topo>(k) == 0) acc[k] = z[k];
	};
	static_for_down<D - kAhead, D>(fetch);
	static_for_down<1, D>([&](auto kc) {
		constexpr int k = decltype(kc)::value;
		// one column per scheduling region (nothing crosses): the ILP scheduler would otherwise hoist the reads and spread the FMAs across the columns, and the
		// substep loop would spill (one column of reads ahead and a full barrier: no scratch access in the substep loop of either instance)
		__builtin_amdgcn_sched_barrier(0);
		if constexpr (k - kAhead >= 1) fetch(std::integral_constant<int, k - kAhead>{});
		const real zk = acc[k];
		if constexpr (first_update_col<Topo>(k) != 0) z[k] = zk;
		static_for_down<0, k>([&](auto ic) {
			constexpr int i = decltype(ic)::value;
			if constexpr (dof_coupled<Topo>(i, k)) acc[i] = fmadd(-u[k * (k - 1) / 2 + i], zk, acc[i]);
		});
	});
	z[0] = acc[0];
}
// x = U^-T u: from DoF 0 down
template <int D>
__device__ __forceinline__ real utsolve_regs(const real (&h)[D], real u)
{
	static_for<0, D - 1>([&](auto kc) {
		constexpr int k = decltype(kc)::value;
		const real uk = bcast(u, k);
		fnma_lanes_ge<k + 1>(u, h[k], uk);              // if (lane > k) u = fma(-h[k], uk, u)
	});
	return u;
}

// contact sample points in registers: lane owns points lane, lane + 64 (, lane + 128); wave ballots give the per-link contact
// flags and the ordered constraint-row list (same order as detect_contacts()/build_rows()) without touching LDS.
// (three named values, not an array: the struct must stay in VGPRs, never in scratch)
// A kernel instance knows its skeleton, hence how many sample points a lane owns: NP = pts_per_lane(Topo::L), two for both shipped skeletons. Everything below is
// instantiated for NP; the fields of the points an instance does not have stay the constants they are initialised with and fold away (no third point's
// zero-init, branch, ballots, link_field() word or row emitter in the physics loop).
static_assert((kMaxPts + kGroup - 1) / kGroup == 3, "written for up to 3 sample points per lane");
constexpr int pts_per_lane(int L) { return (L * kPtsPerLink + kGroup - 1) / kGroup; }
struct ContactPts { PtVal p0, p1, p2; unsigned long long m0, m1, m2; /* constraint-carrying points */ unsigned long long f0, f1, f2; /* points near the surface: contact flags */ };
// the kPtsPerLink ballot bits of link `link`'s sample points (points link * 6 .. link * 6 + 5 of the NP 64-point ballots)
template <int NP>
__device__ __forceinline__ unsigned link_field(unsigned long long m0, unsigned long long m1, unsigned long long m2, int link)
{
	const int b = link * kPtsPerLink, word = b >> 6, off = b & 63;
	unsigned long long lo = m0, hi = NP > 1 ? m1 : 0ull;   // (plain selects on by-value scalars: an indexable aggregate here would be demoted to scratch)
	if constexpr (NP > 1) if (word == 1) { lo = m1; hi = NP > 2 ? m2 : 0ull; }
	if constexpr (NP > 2) if (word == 2) { lo = m2; hi = 0ull; }
	unsigned long long bits = lo >> off;
	if (off + kPtsPerLink > 64) bits |= hi << (64 - off);
	return static_cast<unsigned>(bits & ((1ull << kPtsPerLink) - 1ull));
}
// at most kMaxPtsPerLink constraint-carrying points per link, the deepest ones (ties: lower sample-point index). Cold path (a box lying in the
// ground with five or six of its sample points below the surface): the depths go once through LDS (the packed-matrix storage is dead between
// the factorisation and the Delassus build, and before the controller's mass rows) so that a point sees the other sample points of its link
// Takes and returns scalars only (an aggregate passed by reference to a non-inlined function would live in scratch memory on the hot path):
// d0..d2 = depth of the lane's sample points or kNoPoint when the point carries no rows (a row-carrying point within the breaking threshold above
// the surface has a small negative depth; the points an instance does not have: kNoPoint, not looked at); returns bit k set when point k is dropped
constexpr real kNoPoint = -1.0e30;
template <int NP>
__device__ __noinline__ unsigned link_cap_drop_mask(WSFast& ws, real d0, real d1, real d2)
{
	const int lane = opaque_lane();
	const int npts = ws.M.L * kPtsPerLink;
	real* S = ws.Apk;
	if (lane < npts) S[lane] = d0;
	if constexpr (NP > 1) if (lane + kGroup < npts) S[lane + kGroup] = d1;
	if constexpr (NP > 2) if (lane + 2 * kGroup < npts) S[lane + 2 * kGroup] = d2;
	env_sync();
	auto over = [&](real d, int pt) -> unsigned {
		if (!(d > kNoPoint)) return 0u;
		const int base = (pt / kPtsPerLink) * kPtsPerLink;
		int rank = 0;
		for (int k = 0; k < kPtsPerLink; ++k) { const int o = base + k; const real od = S[o]; rank += (o != pt && (od > d || (od == d && o < pt))) ? 1 : 0; }
		return rank >= kMaxPtsPerLink ? 1u : 0u;
	};
	unsigned m = over(d0, lane);
	if constexpr (NP > 1) m |= over(d1, lane + kGroup) << 1;
	if constexpr (NP > 2) m |= over(d2, lane + 2 * kGroup) << 2;
	env_sync();
	return m;
}
// The ground test of all of a lane's sample points in ONE interleaved pass: contact_point_eval() of dtrl_kernel.h cut into stages, every stage run for all NP
// points before the next one starts. Per point the operations, their operands and their order are exactly contact_point_eval()'s (IEEE division, fmadd where
// it is, nothing reassociated: ground_cell() / ground_height() are the two halves of the one sample_ground()), so the bits are the reference path's.
//   (a) everything that depends on nothing but the lane, issued together: the ground header ONCE (it is the same for every point), and per point the link's
//       collision flag and frame from LDS, its local coordinates, margin and breaking threshold from the model
//   (b) world position, segment pick, grid coordinate, cell indices (ground_cell(): the division is here)
//   (c) the two height loads of every point together
//   (d) gap, margin test, normal, depth, flags
// There is NO branch in here, on purpose. A lane without a point e (pt >= npts) evaluates the last point again, a point of a non-colliding link is evaluated like
// any other (all addresses valid, a NaN coordinate still indexes inside the segment: ground_cell()), and `active` / `near` are SELECTED at the end. With the
// point's evaluation under `if (pt < npts)` and early returns inside, the compiler emits the points strictly one after the other and waits for memory two to three
// times per point -- LDS for the collision flag, the constants + header, the heights, the margins -- which is four to six dependent global round trips and two
// copies of a 65-instruction chain per pass where two trips and one chain at ILP 2 do the same work; the pass runs five times per env-step, all of it on the wave's
// dependent chain. The 1/sqrt of a point that fails the margin test is off that chain and cheap. Do not put the branches back.
// x, y, depth, nx, ny of a point that is not `active` are whatever the evaluation left (nobody reads them: emit_contact_rows(), the drop masks).
// kFlags: also find the points within contact_tol of the surface (the per-link contact flags the controller reads: only the post-step pass needs them)
template <int L, bool kFlags>
__device__ __forceinline__ ContactPts eval_points(WSFast& ws, const DevModel& gm, const GroundRec& g)
{
	constexpr int NP = pts_per_lane(L), npts = L * kPtsPerLink;
	const int lane = opaque_lane();
	// (a)
	const GroundHdr gh = ground_header(g);
	const real q0 = ws.st.q[0], q1 = ws.st.q[1];
	const real tol = kFlags ? gm.contact_tol : real(0);
	bool have[NP]; int col[NP]; real lx[NP], ly[NP], margin[NP], brk[NP], cs[NP], sn[NP], px[NP], py[NP];   // (constant indices only: registers)
	static_for<0, NP>([&](auto ec) {
		constexpr int e = decltype(ec)::value;
		const int pt = lane + e * kGroup;
		have[e] = (e + 1) * kGroup <= npts || pt < npts;
		const int ptc = ((e + 1) * kGroup <= npts || pt < npts) ? pt : npts - 1;
		const int j = ptc / kPtsPerLink;
		col[e] = ws.M.col[j];
		cs[e] = ws.cs[j]; sn[e] = ws.sn[j]; px[e] = ws.px[j]; py[e] = ws.py[j];
		const real* lp = &gm.pt_ground[0][0][0] + 2 * ptc;   // = pt_ground[j][k], k = ptc - j kPtsPerLink: point of the margin-shrunk box
		lx[e] = lp[0]; ly[e] = lp[1];
		margin[e] = gm.link_margin[j]; brk[e] = gm.link_brk[j];
	});
	// every value of stage (a) is pinned here, behind the last of its loads: left alone, the compiler sinks the loads that only the final select reads (the breaking
	// threshold, the collision flag of a lane's last point) into a branch of its own making behind the heights -- a third round trip on the chain
	static_for<0, NP>([&](auto ec) {
		constexpr int e = decltype(ec)::value;
		pin_loaded(col[e]); pin_loaded(lx[e]); pin_loaded(ly[e]); pin_loaded(margin[e]); pin_loaded(brk[e]);
	});
	// (b)
	real x[NP], y[NP]; GroundCell cell[NP];
	static_for<0, NP>([&](auto ec) {
		constexpr int e = decltype(ec)::value;
		x[e] = px[e] + cs[e] * lx[e] - sn[e] * ly[e];
		y[e] = py[e] + sn[e] * lx[e] + cs[e] * ly[e];
		cell[e] = ground_cell(gh, q0 + x[e]);
	});
	// (c)
	real ha[NP], hb[NP];
	static_for<0, NP>([&](auto ec) {
		constexpr int e = decltype(ec)::value;
		ha[e] = g.data[cell[e].seg][cell[e].i];
		hb[e] = g.data[cell[e].seg][cell[e].j];
	});
	// (d)
	PtVal r[3];
	static_for<0, 3>([&](auto ec) {
		constexpr int e = decltype(ec)::value;
		r[e].x = 0; r[e].y = 0; r[e].depth = 0; r[e].nx = 0; r[e].ny = 0; r[e].active = 0; r[e].near = 0;
		if constexpr (e < NP) {
			real slope;
			const real h = ground_height(cell[e], ha[e], hb[e], &slope);
			const real gap = h - (q1 + y[e]);
			// inside a substep only the points that carry rows matter: penetrating ones and -- Bullet's persistent manifold -- those within the breaking threshold above the surface
			// (rows: depth = gap * ny + margin > -brk needs gap > -(margin + brk) / ny, and 1 / ny = sqrt(1 + slope^2) <= 1 + |slope|)
			const bool in_reach = kFlags || (gap + (margin[e] + brk[e]) * (1.0 + fabs(slope)) > 0);
			const real inv = fast_rsqrt(1.0 + slope * slope);
			const real depth = fmadd(gap, inv, margin[e]);   // along the cell normal (ny = inv > 0), to the ROUNDED surface of the box (Bullet's collision margin)
			const bool live = have[e] & (col[e] != 0);   // (& not &&: a select, never a branch)
			if (kFlags) r[e].near = (live & (depth >= -tol)) ? 1 : 0;   // cContactManager::Update: getDistance() <= dist_tol
			r[e].active = (live & in_reach & (depth > -brk[e])) ? 1 : 0;
			r[e].nx = -slope * inv; r[e].ny = inv;
			r[e].depth = depth;
			r[e].x = x[e]; r[e].y = y[e];
		}
	});
	ContactPts c;
	c.p0 = r[0]; c.p1 = r[1]; c.p2 = r[2];
	c.f0 = 0; c.f1 = 0; c.f2 = 0;
	if (kFlags) { c.f0 = __ballot(c.p0.near); if constexpr (NP > 1) c.f1 = __ballot(c.p1.near); if constexpr (NP > 2) c.f2 = __ballot(c.p2.near); }
	c.m0 = __ballot(c.p0.active); c.m1 = 0; c.m2 = 0;
	if constexpr (NP > 1) c.m1 = __ballot(c.p1.active);
	if constexpr (NP > 2) c.m2 = __ballot(c.p2.active);
	if ((c.m0 | c.m1 | c.m2) != 0ull) {   // wave-uniform: somebody penetrates; does any link have more than kMaxPtsPerLink such points?
		const int many = (lane < L) && __popc(link_field<NP>(c.m0, c.m1, c.m2, lane)) > kMaxPtsPerLink;
		if (__builtin_expect(__ballot(many) != 0ull, 0)) {
			const unsigned drop = link_cap_drop_mask<NP>(ws, c.p0.active ? c.p0.depth : kNoPoint, (NP > 1 && c.p1.active) ? c.p1.depth : kNoPoint, (NP > 2 && c.p2.active) ? c.p2.depth : kNoPoint);
			if (drop & 1u) c.p0.active = 0;
			if (drop & 2u) c.p1.active = 0;
			if (drop & 4u) c.p2.active = 0;
			c.m0 = __ballot(c.p0.active);
			if constexpr (NP > 1) c.m1 = __ballot(c.p1.active);
			if constexpr (NP > 2) c.m2 = __ballot(c.p2.active);
		}
	}
	return c;
}
// more penetrating points than constraint rows: the deepest `cap` points overall keep theirs (ties: lower sample-point index). Cold path
// (a character lying on the ground with a dozen points in it)
template <int NP>
__device__ __noinline__ unsigned row_cap_drop_mask(WSFast& ws, real d0, real d1, real d2, int cap)
{
	const int lane = opaque_lane();
	const int npts = ws.M.L * kPtsPerLink;
	real* S = ws.Apk;
	if (lane < npts) S[lane] = d0;
	if constexpr (NP > 1) if (lane + kGroup < npts) S[lane + kGroup] = d1;
	if constexpr (NP > 2) if (lane + 2 * kGroup < npts) S[lane + 2 * kGroup] = d2;
	env_sync();
	auto over = [&](real d, int pt) -> unsigned {
		if (!(d > kNoPoint)) return 0u;
		int rank = 0;
		for (int o = 0; o < npts; ++o) { const real od = S[o]; rank += (o != pt && (od > d || (od == d && o < pt))) ? 1 : 0; }
		return rank >= cap ? 1u : 0u;
	};
	unsigned m = over(d0, lane);
	if constexpr (NP > 1) m |= over(d1, lane + kGroup) << 1;
	if constexpr (NP > 2) m |= over(d2, lane + 2 * kGroup) << 2;
	env_sync();
	return m;
}
// ---- link--link contacts on the wave: one lane per pair decides whether the two boxes can touch at all (hot path: a dozen instructions, almost always
// "no"); the pairs in reach are then taken one at a time, twelve lanes evaluating the twelve candidates (cold path, out of line: nothing of it may
// occupy registers in the physics loop). Same candidates, ranking and row order as append_pair_rows_serial().
__device__ __forceinline__ unsigned long long pairs_in_reach(const WSFast& ws)
{
	const int lane = static_cast<int>(threadIdx.x);
	return __ballot(lane < ws.M.n_cpairs && pair_in_reach(ws, lane));
}
// twelve candidates per pair, five pairs per pass (60 of the 64 lanes): the table reads of a pass travel together, the lane order (pair ascending, candidate
// ascending) is the serial order, so the ballots give the same row positions and the same cut when the row budget runs out.
// When a pair has more than kMaxPtsPerPair penetrating candidates the depth ranking (two barriers, an LDS round trip) only runs when one does.
// (Link--link contacts carry constraint rows but never set a link's contact flag: scenarios/ScenarioSimChar.cpp:321, sim/ContactManager.cpp:169-175.)
constexpr int kPairCands = 2 * kPtsPerLink, kPairSlots = kGroup / kPairCands;
__device__ __noinline__ int append_pair_rows_fast(WSFast& ws, const DevModel& gm, int R, unsigned long long reach)
{
	const int lane = opaque_lane();
	const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
	const int slot = lane / kPairCands, cand = lane - slot * kPairCands;
	while (reach != 0ull && R + 2 <= kMaxRows) {
		int mypr = -1;
#pragma unroll
		for (int sidx = 0; sidx < kPairSlots; ++sidx) {
			if (reach != 0ull) { const int pr = __ffsll(static_cast<long long>(reach)) - 1; reach &= reach - 1ull; if (slot == sidx) mypr = pr; }
		}
		int P = 0, Q = 0, k = 0;
		PairHit hit; hit.active = 0; hit.depth = 0; hit.x = 0; hit.y = 0; hit.nx = 0; hit.ny = 0;
		if (mypr >= 0) { pair_candidate(ws.M.cp_a[mypr], ws.M.cp_b[mypr], cand, &P, &Q, &k); hit = pair_point_eval(ws, gm, P, Q, k); }
		const unsigned long long am = __ballot(hit.active);
		if (am == 0ull) continue;
		int keep = hit.active;
		const int mine_cnt = __popcll((am >> (slot * kPairCands)) & ((1ull << kPairCands) - 1ull));
		if (__builtin_expect(__ballot(lane < kPairSlots * kPairCands && mine_cnt > kMaxPtsPerPair) != 0ull, 0)) {
			real* S = ws.Apk;   // (dead between the factorisation and the Delassus build, like in link_cap_drop_mask())
			S[lane] = hit.active ? hit.depth : -1.0;
			env_sync();
			if (hit.active) {
				int rank = 0;
				for (int o = 0; o < kPairCands; ++o) { const real od = S[slot * kPairCands + o]; rank += (o != cand && od > 0 && (od > hit.depth || (od == hit.depth && o < cand))) ? 1 : 0; }
				keep = rank < kMaxPtsPerPair;
			}
			env_sync();
		}
		const unsigned long long km = __ballot(keep);
		const int room = (kMaxRows - R) / 2;
		const int idx = __popcll(km & below);
		if (keep && idx < room) {
			const int Rw = R + 2 * idx;
			ws.row_kind[Rw] = 1; ws.row_link[Rw] = P; ws.row_link2[Rw] = static_cast<int8_t>(Q); ws.row_x[Rw] = hit.x; ws.row_y[Rw] = hit.y;
			ws.row_dx[Rw] = hit.nx; ws.row_dy[Rw] = hit.ny; ws.row_tgt[Rw] = 0;   // velocity-level only (append_pair_rows_serial)
			ws.row_id[Rw] = pair_row_id(mypr, cand, 0); ws.row_id[Rw + 1] = pair_row_id(mypr, cand, 1);
			ws.row_kind[Rw + 1] = 2; ws.row_link[Rw + 1] = P; ws.row_link2[Rw + 1] = static_cast<int8_t>(Q); ws.row_x[Rw + 1] = hit.x; ws.row_y[Rw + 1] = hit.y;
			ws.row_dx[Rw + 1] = hit.ny; ws.row_dy[Rw + 1] = -hit.nx; ws.row_tgt[Rw + 1] = 0;
		}
		int n = __popcll(km); if (n > room) n = room;
		R += 2 * n;
	}
	return R;
}
template <int NP>
__device__ __forceinline__ void contact_bits_fast(WSFast& ws, unsigned long long m0, unsigned long long m1, unsigned long long m2)
{
	const int lane = static_cast<int>(threadIdx.x);
	int any = 0;
	if (lane < ws.M.L) any = link_field<NP>(m0, m1, m2, lane) != 0u;
	const unsigned long long lm = __ballot(any);
	if (lane == 0) ws.st.contact_bits = static_cast<uint32_t>(lm);
}
__device__ __forceinline__ void emit_contact_rows(WSFast& ws, const PtVal& p, int pt, int rank, int cap, int R0, real inv_h)
{
	if (p.active && rank < cap) {
		const int R = R0 + 2 * rank;
		const int j = pt / kPtsPerLink;
		ws.row_kind[R] = 1; ws.row_link[R] = j; ws.row_link2[R] = -1; ws.row_x[R] = p.x; ws.row_y[R] = p.y;
		ws.row_dx[R] = p.nx; ws.row_dy[R] = p.ny; ws.row_tgt[R] = normal_row_target(p.depth, inv_h);
		ws.row_id[R] = ground_row_id(pt, 0); ws.row_id[R + 1] = ground_row_id(pt, 1);
		ws.row_kind[R + 1] = 2; ws.row_link[R + 1] = j; ws.row_link2[R + 1] = -1; ws.row_x[R + 1] = p.x; ws.row_y[R + 1] = p.y;
		ws.row_dx[R + 1] = p.ny; ws.row_dy[R + 1] = -p.nx; ws.row_tgt[R + 1] = 0;
	}
}
template <int NP>
__device__ __forceinline__ void build_rows_fast(WSFast& ws, const DevModel& gm, const ContactPts& c_in, real h)
{
	ContactPts c = c_in;
	const int lane = opaque_lane();
	const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
	const real inv_h = 1.0 / h;
	// joint limits, ordered by joint id
	int lim = 0; real tgt = 0;
	if (lane >= 1 && lane < ws.M.L && !(ws.M.lim_lo[lane] > ws.M.lim_hi[lane])) {
		const real th = ws.st.q[lane + 2];
		if (th <= ws.M.lim_lo[lane] + kLimitSlop) { lim = 1; tgt = kLimitErp * fmax(ws.M.lim_lo[lane] - th, 0.0) * inv_h; }
		else if (th >= ws.M.lim_hi[lane] - kLimitSlop) { lim = -1; tgt = kLimitErp * fmax(th - ws.M.lim_hi[lane], 0.0) * inv_h; }
	}
	const unsigned long long ml = __ballot(lim != 0);
	const int rl = __popcll(ml & below);
	int R0 = __popcll(ml); if (R0 > kMaxRows) R0 = kMaxRows;
	if (lim != 0 && rl < kMaxRows) { ws.row_kind[rl] = 0; ws.row_link[rl] = lane; ws.row_link2[rl] = -1; ws.row_dx[rl] = lim; ws.row_tgt[rl] = tgt; ws.row_id[rl] = kNoRowId; }
	// contacts, ordered by sample-point index
	const int cap = (kMaxRows - R0) / 2;
	if (__builtin_expect(__popcll(c.m0) + __popcll(c.m1) + __popcll(c.m2) > cap, 0)) {   // wave-uniform
		const unsigned drop = row_cap_drop_mask<NP>(ws, c.p0.active ? c.p0.depth : kNoPoint, (NP > 1 && c.p1.active) ? c.p1.depth : kNoPoint, (NP > 2 && c.p2.active) ? c.p2.depth : kNoPoint, cap);
		if (drop & 1u) c.p0.active = 0;
		if (drop & 2u) c.p1.active = 0;
		if (drop & 4u) c.p2.active = 0;
		c.m0 = __ballot(c.p0.active);
		if constexpr (NP > 1) c.m1 = __ballot(c.p1.active);
		if constexpr (NP > 2) c.m2 = __ballot(c.p2.active);
	}
	const int n0 = __popcll(c.m0), n1 = __popcll(c.m1), n2 = __popcll(c.m2);
	emit_contact_rows(ws, c.p0, lane, __popcll(c.m0 & below), cap, R0, inv_h);
	if constexpr (NP > 1) emit_contact_rows(ws, c.p1, lane + kGroup, n0 + __popcll(c.m1 & below), cap, R0, inv_h);
	if constexpr (NP > 2) emit_contact_rows(ws, c.p2, lane + 2 * kGroup, n0 + n1 + __popcll(c.m2 & below), cap, R0, inv_h);
	int nc = n0 + n1 + n2; if (nc > cap) nc = cap;
	int R = R0 + 2 * nc;
	// link--link contacts take what is left of the row budget
	const unsigned long long reach = pairs_in_reach(ws);
	if (__builtin_expect(reach != 0ull, 0)) R = append_pair_rows_fast(ws, gm, R, reach);
	if (lane == 0) ws.R = R;
	env_sync();
}

// Delassus matrix A = Z D^-1 Z^T, entry-parallel: the R (R + 1) / 2 lower-triangle entries are dealt round-robin to all 64
// lanes (entry e = packed index), so a 16-row system is 3 passes of 23-long dot products instead of 16; the rows of Z are
// read from LDS (odd row stride: lanes on different rows hit different banks, lanes on the same row broadcast).
// Per-entry operation order is the one of build_delassus(), so the bits are the same.
// R: the row count, wave-uniform (FastPath::substep reads it once). Returns the lane's row residual w (lanes >= R: 0), which pgs_solve_fast() takes in a
// register; wv is written all the same (the reference layout).
template <int D>
__device__ __forceinline__ real build_delassus_fast(WSFast& ws, real h, real dinv_mine, int R)
{
	const int lane = static_cast<int>(threadIdx.x);
	const int n_ent = R * (R + 1) / 2;
	if (R < 16) {
		// up to 15 rows (all but 0.2 % of the substeps): [A | zz] = (Z D^-1) Z^T for the R constraint rows plus the free right-hand side as
		// column R is ONE 16x16 tile of the fp64 matrix pipe, six k-steps of v_mfma_f64_16x16x4_f64 (k = DoF, padded to 24). The MFMA
		// accumulates in k order with fused multiply-adds, i.e. the sequence of the scalar loops (tools/microbench/mfma_f64_check.hip).
		// Operand layout: A[i = lane % 16][k = lane / 16], B[k = lane / 16][n = lane % 16], D register r = D[4 r + lane / 16][lane % 16].
		typedef v4r_t v4d_t;
		const int g = lane >> 4, c = lane & 15;
		// row residual's velocity term, on the lanes that finish wv below (independent of the product: overlaps it). Lane r loads ITS row's descriptor as the first
		// substitution does (FastPath::substep) -- kind, links, direction, point, target: one batch, unconditional, clamped -- then the velocity terms of `link` and of
		// max(link2, 0) in a second one, where row_point_jv() makes a trip for the kind, one for the link, one for the point and the link's terms and up to two for
		// link2. link_point_vel() runs for both links; which value counts is selected on the kind and on link2 < 0, and its operations and their order are
		// row_point_jv()'s. (A limit row's point and second direction component hold what an earlier substep left: in bounds, selected away.)
		real jv, tgt;
		{
			const int ol = opaque_lane();
			const int rc = ol < R ? ol : 0;                        // (lanes >= R: row 0 exists, the values are not used)
			const int kind_l = ws.row_kind[rc], link_l = ws.row_link[rc], link2_l = ws.row_link2[rc];
			const real dx_l = ws.row_dx[rc], dy_l = ws.row_dy[rc], x_l = ws.row_x[rc], y_l = ws.row_y[rc];
			tgt = ws.row_tgt[rc];
			const int l2c = link2_l < 0 ? 0 : link2_l;
			const real qd_l = ws.st.qd[link_l + 2];
			const real jv1 = link_point_vel(ws, link_l, x_l, y_l, dx_l, dy_l), jv2 = link_point_vel(ws, l2c, x_l, y_l, dx_l, dy_l);
			const real jp = link2_l < 0 ? jv1 : jv1 - jv2;
			jv = kind_l == 0 ? dx_l * qd_l : jp;
		}
		const int zrow = c <= R ? c : 0;                        // rows above R are never stored; any finite-or-not value will do
		// the twelve operand reads stand in front of the six MFMAs (kin_dyn_terms_fast() P4): counted waits instead of load, wait, MFMA six times over
		constexpr int kSteps = (D + 3) / 4;
		real zv[kSteps], dv[kSteps];
#pragma unroll
		for (int s4 = 0; s4 < kSteps; ++s4) {
			const int k = 4 * s4 + g;
			const bool live = k < D;
			zv[s4] = ws.Z[zrow][live ? k : 0]; dv[s4] = ws.dinv[live ? k : 0];
		}
#pragma unroll
		for (int s4 = 0; s4 < kSteps; ++s4) { pin_loaded(zv[s4]); pin_loaded(dv[s4]); }
		v4d_t acc = {0, 0, 0, 0};
#pragma unroll
		for (int s4 = 0; s4 < kSteps; ++s4) {
			const int k = 4 * s4 + g;
			const bool live = k < D;
			const real b = live ? zv[s4] : 0.0;
			const real a = live ? zv[s4] * dv[s4] : 0.0;
			acc = mfma_16x16x4(a, b, acc);
		}
#pragma unroll
		for (int r = 0; r < 4; ++r) {
			const int i = mfma_row(r, g);                          // D[i][c]
			if (i < R && c <= i) ws.Apk[i * (i + 1) / 2 + c] = acc[r];
			if (i < R && c == R) ws.wv[i] = acc[r];               // zz_i, finished below
		}
		env_sync();
		real w = 0.0;
		if (lane < R) { w = jv + h * ws.wv[lane] - tgt; ws.wv[lane] = w; }
		env_sync();
		return w;
	}
	const real* di = ws.dinv;   // general path (16+ rows, 0.2 % of the substeps): entry-parallel dot products
	auto entry_rows = [](int e, int& s, int& r) {
		s = static_cast<int>((sqrtf(8.0f * e + 1.0f) - 1.0f) * 0.5f);
		while (s * (s + 1) / 2 > e) --s;
		while ((s + 1) * (s + 2) / 2 <= e) ++s;
		r = e - s * (s + 1) / 2;
	};
	// first pass: the lane's matrix entry (all of them for R <= 10) and, on lanes < R, the row's initial residual w = J v_free - target.
	// The two 23-term dot products are independent dependent chains; evaluated in one loop they cost the latency of one
	real w = 0.0;
	{
		const bool has_e = lane < n_ent, has_w = lane < R;
		int s = 0, r = 0;
		if (has_e) entry_rows(lane, s, r);
		const int sw = has_w ? lane : 0;
		real jv = 0;
		if (has_w) {
			if (ws.row_kind[sw] == 0) jv = ws.row_dx[sw] * ws.st.qd[ws.row_link[sw] + 2];
			else jv = row_point_jv(ws, sw);
		}
		const real* zs = ws.Z[s];
		const real* zr = ws.Z[r];
		const real* zw = ws.Z[sw];
		const real* z0 = ws.Z[R];
		real a = 0, zz = 0;
#pragma unroll 4
		for (int i = 0; i < D; ++i) { a = fmadd(zs[i] * di[i], zr[i], a); zz = fmadd(zw[i] * di[i], z0[i], zz); }
		if (has_e) ws.Apk[lane] = a;
		if (has_w) { w = jv + h * zz - ws.row_tgt[lane]; ws.wv[lane] = w; }
	}
	for (int e = lane + kGroup; e < n_ent; e += kGroup) {
		int s, r; entry_rows(e, s, r);
		const real* zs = ws.Z[s];
		const real* zr = ws.Z[r];
		real a = 0;
#pragma unroll 4
		for (int i = 0; i < D; ++i) a = fmadd(zs[i] * di[i], zr[i], a);
		ws.Apk[e] = a;
	}
	env_sync();
	return w;
}

// projected Gauss-Seidel in lambda space with the row state in registers: lane s owns row s (w_s, lambda_s, 1/A_ss, kind).
// The solve is one long dependent chain (10 sweeps x R row updates): the number of DEPENDENT instructions per update matters -- and, with two waves per SIMD, so does the
// instruction count (round 5: the 27-instruction generic step was issue-bound; the per-pass steps below are 9-11). Every lane evaluates its own candidate update each step (lane r's is the one that
// counts): the projection bounds [lo, hi] (normal rows [0, inf), tangent rows +-mu * lambda of the row before it, fetched with
// a wave_shr:1 DPP move) are off the chain, leaving w -> mul -> sub -> max -> min -> sub -> readlane -> mul -> add.
// Same operations on the same operands as pgs_solve(), hence the same bits; rows with a vanishing effective mass are skipped.
__device__ __forceinline__ real wave_shr1(real v)
{
#if defined(DTRL_REAL_F32)
	return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));   // DPP wave_shr:1
#else
	const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(v), 0x138, 0xf, 0xf, false);   // DPP wave_shr:1
	const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(v), 0x138, 0xf, 0xf, false);
	return __hiloint2double(hi, lo);
#endif
}
// ONE row update of the Gauss-Seidel chain, the only spelling of it: project lane r's candidate, broadcast its delta, apply it to every lane's residual through the
// lane's Delassus entry a_sr = A(lane, r). The unrolled sequences and the plain loop of pgs_solve_fast() all call it, which is what keeps them -- and pgs_solve() of
// dtrl_kernel.h -- on the same bits. The kinds differ in the projection only:
//   kPgsRowNormal    limit and normal rows, onto [0, inf): fma, max, sub, readlane, fma
//   kPgsRowFriction  friction rows that are not held, onto [lo, hi] = +-mu lambda_n, LANE REGISTERS set once per pass (every normal row is final for the sweep by then):
//                    fma, max, min, sub, readlane, fma
//   kPgsRowGeneric   the row step of rounds 1-4, bounds evaluated per step (normal rows [0, inf), tangent rows +-mu * lambda of the row before it, a DPP move, a multiply,
//                    a compare and selects more than the two above). Only -warm_start= 0 (the round-4 contact model, an ablation) still runs it.
//                    (A wave-uniform branch on the kind of row r instead of the selects was measured twice, round 1 and round 4 under the ILP scheduler: -6 % / -3 %.)
enum PgsRowKind { kPgsRowNormal, kPgsRowFriction, kPgsRowGeneric };
template <PgsRowKind kKind>
__device__ __forceinline__ void pgs_row_step(real& w, real& lam, real rinv, real a_sr, int r, int lane, bool tang, real lo, real hi)
{
	real nl;
	if constexpr (kKind == kPgsRowGeneric) {
		const real lim = kMu * wave_shr1(lam);
		const real glo = tang ? -lim : 0.0, ghi = tang ? lim : __builtin_huge_val();
		nl = fmin(fmax(fmadd(-w, rinv, lam), glo), ghi);
	} else {
		nl = fmadd(-w, rinv, lam);
		if constexpr (kKind == kPgsRowFriction) nl = fmin(fmax(nl, lo), hi); else nl = fmax(nl, 0.0);   // (pgs_solve(): normal and limit rows are projected onto [0, inf))
	}
	const real dl = bcast(nl - lam, r);
	if (lane == r) lam = nl;
	w = fmadd(a_sr, dl, w);
}
// The unrolled row sequences (substeps with up to K rows, the lane's Delassus row in registers). They are NESTED (row r + 1 sits inside `if (r < R)` of row r), so a
// substep leaves them at its first absent row with one scalar compare + branch per row that exists: tested row by row, the absent rows cost 4 dependent SALU
// instructions each, ten sweeps per substep -- +4 k cycles on the typical substep with 3 rows (round 4).
// a[r] = A(lane, r) for the rows that exist
template <int r, int K>
__device__ __forceinline__ void pgs_rows_load(real (&a)[K], const WSFast& ws, int lane, bool mine, int R)
{
	if constexpr (r < K) {
		if (r < R) {
			const int mx = lane > r ? lane : r, mn = lane < r ? lane : r;
			a[r] = ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0];
			pgs_rows_load<r + 1, K>(a, ws, lane, mine, R);
		}
	}
}
// -warm_start= 0: one interleaved sweep over the rows r, r + 1, ... of actR
template <int r, int K>
__device__ __forceinline__ void pgs_rows_sweep(const real (&a)[K], real& w, real& lam, real rinv, bool tang, unsigned long long actR, int lane, int R)
{
	if constexpr (r < K) {
		if (r < R) {
			if ((actR >> r) & 1ull) pgs_row_step<kPgsRowGeneric>(w, lam, rinv, a[r], r, lane, tang, 0.0, 0.0);
			pgs_rows_sweep<r + 1, K>(a, w, lam, rinv, tang, actR, lane, R);
		}
	}
}
// one of the two passes of a sweep under Bullet's contact persistence (round 5) over the rows r, r + 1, ... of `rows`
template <PgsRowKind kKind, int r, int K>
__device__ __forceinline__ void pgs_rows_pass(const real (&a)[K], real& w, real& lam, real rinv, real lo, real hi, unsigned long long rows, int lane, int R)
{
	if constexpr (r < K) {
		if (r < R) {
			if ((rows >> r) & 1ull) pgs_row_step<kKind>(w, lam, rinv, a[r], r, lane, false, lo, hi);
			pgs_rows_pass<kKind, r + 1, K>(a, w, lam, rinv, lo, hi, rows, lane, R);
		}
	}
}
// w += A lambda_0 (the warm-started impulses), column by column in row order: the same fused operations as pgs_solve()'s first loop
template <int r, int K>
__device__ __forceinline__ void pgs_rows_warm(const real (&a)[K], real& w, real lam, unsigned long long nz, int R)
{
	if constexpr (r < K) {
		if (r < R) {
			if ((nz >> r) & 1ull) w = fmadd(a[r], bcast(lam, r), w);   // (rows that start from zero -- limit rows, link--link rows, new contacts -- add exactly nothing)
			pgs_rows_warm<r + 1, K>(a, w, lam, nz, R);
		}
	}
}
// ---- the two passes of a sweep under Bullet's contact persistence, each walking ITS OWN rows only ----
// The list is limit rows followed by (normal, tangent) pairs, so in row order each pass steps over the other pass's slots: three scalar instructions for "is this slot
// in this pass" and three for "was this the last", around nine to ten of a row step. Here the lane's Delassus entries sit in SLOT order: the rows of pass 0 (limit and
// normal rows that are active) take slots 0, 1, ... in list order, the rows of pass 1 (active friction rows) take slots K - 1, K - 2, ... in list order. A pass enters
// its nested sequence at a compile-time slot and leaves at its first absent one: one scalar compare and branch per executed step. Lane ownership does not change (lane s
// owns row s: w, lambda, 1/A_ss, kind), so wave_shr1(lam) and the final store stay; the row of a slot is wave-uniform, read from lane `slot` of one VGPR (srow) that is
// built once per solve, and a step broadcasts from that row and commits on `lane == row` against the scalar. Same operations on the same operands in the same order per
// lane as in row order, i.e. as pgs_solve().
__device__ __forceinline__ real pgs_slot_entry(const WSFast& ws, int lane, bool mine, int row)
{
	const int mx = lane > row ? lane : row, mn = lane < row ? lane : row;
	return ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0];
}
// a[slot] = A(lane, row(slot)) for the n0 slots from 0 up and the n1 slots from K - 1 down
template <int j, int K>
__device__ __forceinline__ void pgs_slots_load_up(real (&a)[K], const WSFast& ws, int lane, bool mine, int srow, int n0)
{
	if constexpr (j < K) {
		if (j < n0) {
			a[j] = pgs_slot_entry(ws, lane, mine, __builtin_amdgcn_readlane(srow, j));
			pgs_slots_load_up<j + 1, K>(a, ws, lane, mine, srow, n0);
		}
	}
}
template <int j, int K>
__device__ __forceinline__ void pgs_slots_load_down(real (&a)[K], const WSFast& ws, int lane, bool mine, int srow, int n1)
{
	if constexpr (j < K) {
		if (j < n1) {
			a[K - 1 - j] = pgs_slot_entry(ws, lane, mine, __builtin_amdgcn_readlane(srow, K - 1 - j));
			pgs_slots_load_down<j + 1, K>(a, ws, lane, mine, srow, n1);
		}
	}
}
// pass 0: slots 0 .. n0 - 1
template <int j, int K>
__device__ __forceinline__ void pgs_slots_pass0(const real (&a)[K], real& w, real& lam, real rinv, int lane, int srow, int n0)
{
	if constexpr (j < K) {
		if (j < n0) {
			pgs_row_step<kPgsRowNormal>(w, lam, rinv, a[j], __builtin_amdgcn_readlane(srow, j), lane, false, 0.0, 0.0);
			pgs_slots_pass0<j + 1, K>(a, w, lam, rinv, lane, srow, n0);
		}
	}
}
// pass 1: slots K - 1 .. K - n1. A friction row that Bullet's rule holds in this sweep (its bit of `rows` clear) must not run: fma(a, +-0, w) can change the sign of a zero
template <int j, int K>
__device__ __forceinline__ void pgs_slots_pass1(const real (&a)[K], real& w, real& lam, real rinv, real lo, real hi, int lane, int srow, int n1, unsigned long long rows)
{
	if constexpr (j < K) {
		if (j < n1) {
			const int row = __builtin_amdgcn_readlane(srow, K - 1 - j);
			if ((rows >> row) & 1ull) pgs_row_step<kPgsRowFriction>(w, lam, rinv, a[K - 1 - j], row, lane, false, lo, hi);
			pgs_slots_pass1<j + 1, K>(a, w, lam, rinv, lo, hi, lane, srow, n1, rows);
		}
	}
}
// Bullet's persistent contact points on the wave (warm_match() of dtrl_kernel.h): lane r looks the identity of fresh row r up among the rows of the last solved
// substep and starts from kWarmFactor x that row's impulse; the fresh list then becomes the cache. Lane p loads cached id p in the same batch as its own row's id, and
// the loop over the cache takes id p from lane p (v_readlane, wave-uniform p) instead of one broadcast LDS read, wait and compare per cached row; the select is the
// same, so the same -- last -- match wins. The impulse of the hit is the one dependent trip left.
// R, Rp (row count of the last solved substep), warm (DevModel::warm_start): wave-uniform, read once by FastPath::substep
__device__ __forceinline__ void warm_match_fast(WSFast& ws, int R, int Rp, bool warm)
{
	const int lane = opaque_lane();
	if (R == 0) { if (Rp != 0 && lane == 0) ws.st.ws_R = 0; return; }   // (a fifth of the substeps: airborne)
	const int own = ws.row_id[lane < R ? lane : 0];
	const int cached = ws.st.ws_id[lane < Rp ? lane : 0];   // (Rp = 0: entry 0 is in bounds and not looked at)
	const int id = lane < R ? own : kNoRowId;
	real l0 = 0.0;
	if (warm && Rp > 0) {
		int hit = -1;
		for (int p = 0; p < Rp; ++p) hit = (__builtin_amdgcn_readlane(cached, p) == id) ? p : hit;
		const real lh = ws.st.ws_lam[hit >= 0 ? hit : 0];
		if (id < kFirstPairRowId && hit >= 0) l0 = kWarmFactor * lh;   // ground contact rows only
	}
	// (no barrier between the reads above and the writes below: one wavefront, and its LDS operations complete in issue order)
	if (lane < R) { ws.st.ws_lam[lane] = l0; ws.st.ws_id[lane] = static_cast<uint16_t>(id); }
	if (lane == 0) ws.st.ws_R = R;
	// (no fence behind the writes either: their next reader is the Gauss-Seidel solve, several phase boundaries further on)
}
// R, warm: wave-uniform (FastPath::substep); w: the lane's row residual from build_delassus_fast() (lanes >= R: 0)
// kSlotOrder: the two passes of a sweep walk their own rows in slot order (pgs_slots_pass0() / pgs_slots_pass1() above); false: the row-order sequences
template <int kPgsRegRows, bool kSlotOrder>
__device__ __forceinline__ void pgs_solve_fast(WSFast& ws, int R, bool warm, real w)
{
	const int lane = opaque_lane();
	const bool mine = lane < R;
	// the diagonal entry, the warm-start impulse and the row kind in one batch (unconditional, clamped: lanes >= R read row 0's)
	const int rc = mine ? lane : 0;
	const real ass = ws.Apk[rc * (rc + 3) / 2], lam_ws = ws.st.ws_lam[rc];
	const int kind = ws.row_kind[rc];
	real rinv = 0.0;
	if (mine) rinv = (ass >= 1e-12) ? 1.0 / ass : 0.0;
	real lam = (mine && rinv != 0.0) ? lam_ws : 0.0;   // warm_match_fast(): kWarmFactor x the row's previous impulse; rows with a vanishing effective mass stay at zero
	const bool tang = mine && kind == 2;
	const unsigned long long act = __ballot(rinv != 0.0);
	// Bullet's contact persistence: a sweep resolves the limit and normal rows (list order), then the friction rows; a friction row only under a loaded normal row
	const unsigned long long tmask = __ballot(tang);
	const unsigned long long nz_l0 = __ballot(lam != 0.0);
	const bool any_l0 = nz_l0 != 0ull;
	// Substeps with up to kPgsRegRows rows (per skeleton, dtrl_topo.h: every substep of the dog's instance) keep the lane's Delassus row in registers for all sweeps
	// -- no LDS read and no packed-index arithmetic per row update -- and run the unrolled, nested row sequences. Same operations on the same values in the same order
	// as pgs_solve() of dtrl_kernel.h. The rare substeps with many rows matter out of proportion: they are what the slowest envs of a launch do in EVERY substep (a
	// character lying on the ground), and a launch lasts as long as its slowest env.
	// (the first test is a compile-time constant: an instance whose register rows cover every row count does not contain the plain loop)
	if (kPgsRegRows == kMaxRows || R <= kPgsRegRows) {
		real a[kPgsRegRows];
		if (!kSlotOrder || !warm || any_l0) pgs_rows_load<0, kPgsRegRows>(a, ws, lane, mine, R);   // row order: the warm-start columns, the -warm_start= 0 sweep, the instances that keep the row-order passes
		// every a[r] has arrived here, once per solve: the nested loads leave at R different depths, and without this wait the FMA of every row step of both passes
		// gets an s_waitcnt lgkmcnt(0) of its own (docs/EXPERIMENTS.md 38)
		lds_loads_arrived();
		const unsigned long long actR = act & ((R < 64) ? ((1ull << R) - 1ull) : ~0ull);
		if (any_l0) pgs_rows_warm<0, kPgsRegRows>(a, w, lam, nz_l0, R);
		const unsigned long long pass0 = warm ? (actR & ~tmask) : actR, pass1 = actR & tmask;
		if (warm) {
			if constexpr (kSlotOrder) {
				// (w += A lambda_0 above ran on the entries in ROW order, column by column in list order as pgs_solve() does; the same registers now take them in slot order.
				// A solve with a warm impulse therefore reads the lane's Delassus row twice, two batches and two waits; reading the warm-start columns straight from Apk
				// instead needs R more live registers next to a[] or a second nest of loads, and was not built: docs/EXPERIMENTS.md 38 "Not done")
				const int n0 = __popcll(pass0), n1 = __popcll(pass1);
				int srow;
				{
					// lane r knows the slot of row r (its rank in its pass); one cross-lane push turns that into slot -> row. Lanes without a slot push to lane 63, which no
					// slot uses (K <= kMaxRows < 63)
					const unsigned long long below = (1ull << lane) - 1ull;
					const bool has = ((actR >> lane) & 1ull) != 0ull;
					const int slot = tang ? kPgsRegRows - 1 - __popcll(pass1 & below) : __popcll(pass0 & below);
					srow = __builtin_amdgcn_ds_permute((has ? slot : 63) << 2, lane);
				}
				pgs_slots_load_up<0, kPgsRegRows>(a, ws, lane, mine, srow, n0);
				pgs_slots_load_down<0, kPgsRegRows>(a, ws, lane, mine, srow, n1);
				lds_loads_arrived();   // (as above: every entry has arrived before the sweeps)
#pragma unroll 1
				for (int it = 0; it < kPgsIters; ++it) {
					// n0 / n1 / srow do not change over the sweeps. Left visible as loop invariants, the per-slot tests and row indices are hoisted out of the loop into SGPRs
					// that do not exist (they spill to VGPR lanes and every row of every sweep reads them back): through an opaque per-sweep copy they are formed where they are used
					int n0s = n0, n1s = n1, srows = srow;
					asm volatile("" : "+s"(n0s), "+s"(n1s), "+v"(srows));
					pgs_slots_pass0<0, kPgsRegRows>(a, w, lam, rinv, lane, srows, n0s);
					// friction pass: every normal row is final for this sweep, so the bounds +-mu lambda_n are fixed for the pass, and which friction rows Bullet's rule HOLDS
					// (normal row without impulse: their update is exactly zero) is known up front
					const real ln = wave_shr1(lam);   // (all lanes: a DPP move under a narrowed EXEC does not see the lanes that are switched off)
					const real lim = kMu * ln;
					const unsigned long long rows = pass1 & __ballot(tang && ln > kHoldEps);
					if (rows != 0ull) pgs_slots_pass1<0, kPgsRegRows>(a, w, lam, rinv, -lim, lim, lane, srows, n1s, rows);
				}
			} else {
				// a pass leaves the nested row sequence behind its LAST row (not at R): the rows of the other pass that follow it are not even looked at
				const int end0 = (pass0 == 0ull) ? R : 64 - __builtin_clzll(pass0);
#pragma unroll 1
				for (int it = 0; it < kPgsIters; ++it) {
					// pass0 / end0 do not change over the sweeps. Left visible as loop invariants, the nested per-row tests below are hoisted out of the loop as two
					// 64-bit booleans per row, which have no SGPRs to live in: a block in front of every solve writes them to VGPR lanes and every row of every
					// sweep reads them back. Through an opaque per-sweep copy they are tested where they are used, as the friction pass's per-sweep `rows` is:
					// s_cmp / s_bitcmp + branch per row, nothing kept.
					// (the mask travels as two 32-bit halves: with a 64-bit operand next to the 32-bit one the fp32 build does not compile)
					unsigned rows0_lo = static_cast<unsigned>(pass0), rows0_hi = static_cast<unsigned>(pass0 >> 32); int last0 = end0;
					asm volatile("" : "+s"(rows0_lo), "+s"(rows0_hi), "+s"(last0));
					const unsigned long long rows0 = (static_cast<unsigned long long>(rows0_hi) << 32) | rows0_lo;
					if (rows0 != 0ull) pgs_rows_pass<kPgsRowNormal, 0, kPgsRegRows>(a, w, lam, rinv, 0.0, 0.0, rows0, lane, last0);
					// friction pass: every normal row is final for this sweep, so the bounds +-mu lambda_n are fixed for the pass, and which friction rows Bullet's rule HOLDS
					// (normal row without impulse: their update is exactly zero) is known up front -- they leave the pass instead of walking through a row step each
					const real ln = wave_shr1(lam);   // (all lanes: a DPP move under a narrowed EXEC does not see the lanes that are switched off)
					const real lim = kMu * ln;
					const unsigned long long rows = pass1 & __ballot(tang && ln > kHoldEps);
					if (rows != 0ull) pgs_rows_pass<kPgsRowFriction, 0, kPgsRegRows>(a, w, lam, rinv, -lim, lim, rows, lane, 64 - __builtin_clzll(rows));
				}
			}
		} else {
#pragma unroll 1
			for (int it = 0; it < kPgsIters; ++it) {
				// (actR / R through an opaque per-sweep copy, as pass0 / end0 above. The fp32 build keeps R visible: with it opaque as well, the 168-VGPR raptor
				// instance of the external-policy kernel gets six scratch reloads in its substep loop)
				unsigned rows_lo = static_cast<unsigned>(actR), rows_hi = static_cast<unsigned>(actR >> 32); int last = R;
#if defined(DTRL_REAL_F32)
				asm volatile("" : "+s"(rows_lo), "+s"(rows_hi));
#else
				asm volatile("" : "+s"(rows_lo), "+s"(rows_hi), "+s"(last));
#endif
				pgs_rows_sweep<0, kPgsRegRows>(a, w, lam, rinv, tang, (static_cast<unsigned long long>(rows_hi) << 32) | rows_lo, lane, last);
			}
		}
		if (mine) ws.st.ws_lam[lane] = lam;
		env_sync();
		return;
	}
	// more rows than register rows: the plain loop, the lane's entry of the next row update's column fetched from LDS one update ahead
	// (the fetch is written out in each of the three loops: folded into a helper or a lambda, both instances of the kernel come out with a different register allocation)
	const int tri = lane * (lane + 1) / 2;
	if (any_l0) for (int r = 0; r < R; ++r) if ((nz_l0 >> r) & 1ull) { const int mx = lane > r ? lane : r, mn = lane < r ? lane : r; w = fmadd(ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0], bcast(lam, r), w); }
	real a_nx = mine ? ws.Apk[tri] : 0.0;   // column 0
	const unsigned long long actR = act & ((R < 64) ? ((1ull << R) - 1ull) : ~0ull);
	if (warm) {
		const unsigned long long pass0 = actR & ~tmask, pass1 = actR & tmask;
		for (int it = 0; it < kPgsIters; ++it) {
			for (int r = 0; r < R; ++r) {
				const real a_sr = a_nx;
				const int rn = (r + 1 < R) ? r + 1 : 0;
				{ const int mx = lane > rn ? lane : rn, mn = lane < rn ? lane : rn; a_nx = ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0]; }   // branch-free packed index
				if (!((pass0 >> r) & 1ull)) continue;
				pgs_row_step<kPgsRowNormal>(w, lam, rinv, a_sr, r, lane, false, 0.0, 0.0);
			}
			const real ln = wave_shr1(lam);
			const real lim = kMu * ln;
			const unsigned long long rows = pass1 & __ballot(tang && ln > kHoldEps);
			for (int r = 0; r < R; ++r) {
				const real a_sr = a_nx;
				const int rn = (r + 1 < R) ? r + 1 : 0;
				{ const int mx = lane > rn ? lane : rn, mn = lane < rn ? lane : rn; a_nx = ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0]; }
				if (!((rows >> r) & 1ull)) continue;
				pgs_row_step<kPgsRowFriction>(w, lam, rinv, a_sr, r, lane, false, -lim, lim);
			}
		}
	} else {
		for (int it = 0; it < kPgsIters; ++it) {
			for (int r = 0; r < R; ++r) {
				const real a_sr = a_nx;
				const int rn = (r + 1 < R) ? r + 1 : 0;
				{ const int mx = lane > rn ? lane : rn, mn = lane < rn ? lane : rn; a_nx = ws.Apk[mine ? mx * (mx + 1) / 2 + mn : 0]; }   // branch-free packed index
				if (!((act >> r) & 1ull)) continue;
				pgs_row_step<kPgsRowGeneric>(w, lam, rinv, a_sr, r, lane, tang, 0.0, 0.0);
			}
		}
	}
	if (mine) ws.st.ws_lam[lane] = lam;
	env_sync();
}

// kin_dyn_terms() of dtrl_kernel.h for a compiled-in skeleton: what substeps 2..n and the post-step evaluation of an env-step run (the cold evaluations -- frame start,
// reset, resume -- keep the generic function). Every term that is "on" goes through the same operations on the same values in the same order, and every workspace
// array the generic function writes is written; what changes is how the operands arrive. The generic function reads one path element, waits, adds, 12 and 11 times
// over, re-reads from LDS what the lane itself produced a phase earlier, and opens every phase with a load of M.L and a branch: about 45 dependent LDS round trips per
// evaluation. Here
//   - the lane's path words, depth, parent, subtree-mask words and model constants arrive in ONE batch at the head, q / qd of the whole path in a second one;
//   - the lane's own cs, sn, w (P1 -> P3), px, py (P3 -> bias) and the mask words (head -> P4) stay in registers;
//   - P3's bone gather is issued in counted batches of kKinBatch path elements, the sums of one batch running under the loads of the next;
//   - P4's six operand reads stand in front of the MFMAs;
//   - the link count and the loop lengths are Topo's (topo_depth()), not M.L and kMaxDepth.
// What still goes through LDS: the parent's cs / sn / w (P2), the bone gather (P3), the operands and the result layout of the subtree product (P4).
// The dropped iterations topo_depth() .. kMaxDepth - 1 are exact: on every lane the generic function adds x * 0.0 there with x = q[2] / qd[2] (P1: finite) or link 0's
// bone terms (P3: +0, the root has no parent), i.e. +-0 or +0 to the accumulator. An accumulator that started at +0 (phi, w, px, py, ax, ay) is never -0 under
// round-to-nearest, so adding a zero of either sign leaves it as it is. vx, vy start at qd[0], qd[1] and can be -0 when every live term is -0; the generic function's
// first dropped iteration turns that into -0 + +0 = +0 and the later ones keep it, which is what ONE `+ 0.0` does here (it is the identity on everything else, and on the
// lanes whose path is shorter, where a masked iteration has already done it). Lanes >= Topo::L evaluate link 0 and store nothing.
// Force-inlined at its two call sites (FastPath::substep, FastPath::kinematics). One __noinline__ instance per skeleton was measured too: the dog's uses 248 VGPRs and
// saves twelve callee registers to scratch per call, and it gains half of what this form gains (docs/EXPERIMENTS.md 34).
constexpr int kKinBatch = 3;   // path elements per batch of P3: 18 values in flight next to the 18 being summed (dog: 3 + 3 + 3, raptor: 3 + 2)
template <class Topo>
__device__ __forceinline__ void kin_dyn_terms_fast(WSFast& ws)
{
	constexpr int L = Topo::L, kDepth = topo_depth<Topo>();
	static_assert(kDepth >= 2 && kDepth <= kMaxDepth, "path length of the skeleton against the model's path table");
	constexpr int kWords = (kDepth + 3) / 4;
	PROF_T0();
	const int lane = opaque_lane();
	const bool mine = lane < L;
	const int j = mine ? lane : 0;
	// ---- head: everything that is addressed by the lane id alone, one batch
	const int dep = ws.M.depth[j], pa = ws.M.parent[j];
	uint32_t pw[kWords];
#pragma unroll
	for (int t = 0; t < kWords; ++t) pw[t] = path_word(ws, j, t);
	const int mc = lane & 15;
	const uint32_t m0_l = ws.M.sub_mask[mc < L ? mc : 0], m1_l = ws.M.sub_mask[16 + mc < L ? 16 + mc : 0];   // rows mc and 16 + mc of the mask matrix (P4)
	const real at0 = ws.M.attach[j][0], at1 = ws.M.attach[j][1], ba0 = ws.M.body_attach[j][0], ba1 = ws.M.body_attach[j][1];
	const real m = ws.M.mass[j], inr = ws.M.inertia[j], subm = ws.M.sub_mass[j];
	int a[kDepth];
#pragma unroll
	for (int k = 0; k < kDepth; ++k) a[k] = (k <= dep) ? static_cast<int>((pw[k / 4] >> (8 * (k % 4))) & 0xffu) : 0;
	// ---- P1: q, qd of the path in one batch
	real qa[kDepth], wa[kDepth];
#pragma unroll
	for (int k = 0; k < kDepth; ++k) { qa[k] = ws.st.q[a[k] + 2]; wa[k] = ws.st.qd[a[k] + 2]; }
	const real vx0 = ws.st.qd[0], vy0 = ws.st.qd[1];
#pragma unroll
	for (int k = 0; k < kDepth; ++k) { pin_loaded(qa[k]); pin_loaded(wa[k]); }
	real phi = 0, w = 0;
#pragma unroll
	for (int k = 0; k < kDepth; ++k) {
		const real on = (k <= dep) ? 1.0 : 0.0;
		phi = fmadd(qa[k], on, phi); w = fmadd(wa[k], on, w);
	}
	real sn, cs; sincos_r(phi, &sn, &cs);
	if (mine) { ws.phi[j] = phi; ws.w[j] = w; ws.cs[j] = cs; ws.sn[j] = sn; }
	env_sync();
	PROF_ADD(ws, kProfP1);
	// ---- P2: the bone vector of the link from the parent's angle and rate
	{
		const int pc = pa >= 0 ? pa : 0;
		const real c = ws.cs[pc], s = ws.sn[pc], wp = ws.w[pc];
		const real rx = c * at0 - s * at1;
		const real ry = s * at0 + c * at1;
		const real ux = -(wp * ry), uy = wp * rx;
		const real w2 = wp * wp;
		const real gx = -(w2 * rx), gy = -(w2 * ry);
		const bool has = pa >= 0;
		if (mine) {
			ws.bx[j] = has ? rx : 0.0; ws.by[j] = has ? ry : 0.0; ws.ux[j] = has ? ux : 0.0; ws.uy[j] = has ? uy : 0.0; ws.gx[j] = has ? gx : 0.0; ws.gy[j] = has ? gy : 0.0;
		}
	}
	env_sync();
	PROF_ADD(ws, kProfP2);
	// ---- P3: sums of the bone terms along the path, in counted batches (the loads of batch i + 1 are in flight while batch i is summed)
	real px = 0, py = 0, vx = vx0, vy = vy0, ax = 0, ay = 0;
	{
		constexpr int kN = kDepth - 1;                      // path elements 1 .. kDepth - 1
		real v[kN][6];
		auto load = [&](int k) {                            // element k sits in v[k - 1]
			const int e = a[k];
			v[k - 1][0] = ws.bx[e]; v[k - 1][1] = ws.by[e]; v[k - 1][2] = ws.ux[e]; v[k - 1][3] = ws.uy[e]; v[k - 1][4] = ws.gx[e]; v[k - 1][5] = ws.gy[e];
		};
#pragma unroll
		for (int k = 1; k <= (kKinBatch < kN ? kKinBatch : kN); ++k) load(k);
		__builtin_amdgcn_sched_barrier(0);                  // (the scheduler otherwise interleaves the batches' loads, and the first wait drains them all)
#pragma unroll
		for (int b0 = 1; b0 <= kN; b0 += kKinBatch) {
#pragma unroll
			for (int k = b0 + kKinBatch; k < b0 + 2 * kKinBatch && k <= kN; ++k) load(k);
			__builtin_amdgcn_sched_barrier(0);
#pragma unroll
			for (int k = b0; k < b0 + kKinBatch && k <= kN; ++k) {
#pragma unroll
				for (int t = 0; t < 6; ++t) pin_loaded(v[k - 1][t]);
			}
#pragma unroll
			for (int k = b0; k < b0 + kKinBatch && k <= kN; ++k) {
				const real on = (k <= dep) ? 1.0 : 0.0;
				px = fmadd(v[k - 1][0], on, px); py = fmadd(v[k - 1][1], on, py); vx = fmadd(v[k - 1][2], on, vx); vy = fmadd(v[k - 1][3], on, vy);
				ax = fmadd(v[k - 1][4], on, ax); ay = fmadd(v[k - 1][5], on, ay);
			}
		}
		if constexpr (kDepth < kMaxDepth) { vx = vx + 0.0; vy = vy + 0.0; }   // the generic function's dropped iterations (above)
	}
	{
		const real ax0 = 0, ay0 = -kGravityY;
		const real rx = cs * ba0 - sn * ba1;
		const real ry = sn * ba0 + cs * ba1;
		const real cx = px + rx, cy = py + ry;
		const real w2 = w * w;
		const real fx = m * ((ax0 + ax) - w2 * rx), fy = m * ((ay0 + ay) - w2 * ry);
		if (mine) {
			ws.px[j] = px; ws.py[j] = py; ws.vpx[j] = vx; ws.vpy[j] = vy;
			ws.cx[j] = cx; ws.cy[j] = cy;
			ws.vcx[j] = vx - w * ry; ws.vcy[j] = vy + w * rx;
			ws.fx[j] = fx; ws.fy[j] = fy; ws.fn[j] = cx * fy - cy * fx;
			ws.mcx[j] = m * cx; ws.mcy[j] = m * cy; ws.Io[j] = inr + m * (cx * cx + cy * cy);
		}
	}
	env_sync();
	PROF_ADD(ws, kProfP3);
	// ---- P4: the subtree sums on the matrix pipe (kin_dyn_terms(): same operands, same k order), the six operand reads in front of the MFMAs
	{
		const int g = lane >> 4, c = lane & 15;
		const real* V = &ws.fx[0];
		const uint32_t m0 = (c < L) ? m0_l : 0u, m1 = (16 + c < L) ? m1_l : 0u;
		real bv[kMaxL / 4];
#pragma unroll
		for (int s4 = 0; s4 < kMaxL / 4; ++s4) {
			const int k = 4 * s4 + g;
			const bool live = (c < 6) & (k < L);                                  // never multiply an unwritten LDS slot, not even by zero
			bv[s4] = V[live ? c * kMaxL + k : 0];
		}
#pragma unroll
		for (int s4 = 0; s4 < kMaxL / 4; ++s4) pin_loaded(bv[s4]);
		v4r_t acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
#pragma unroll
		for (int s4 = 0; s4 < kMaxL / 4; ++s4) {
			const int k = 4 * s4 + g;
			const bool live = (c < 6) & (k < L);
			const real b = live ? bv[s4] : 0.0;
			const real a0 = ((m0 >> k) & 1u) ? 1.0 : 0.0, a1 = ((m1 >> k) & 1u) ? 1.0 : 0.0;
			acc0 = mfma_16x16x4(a0, b, acc0);
			acc1 = mfma_16x16x4(a1, b, acc1);
		}
		if (c < 6) {
			real* out = (c < 3) ? &ws.sfs[c][0] : (&ws.smx[0] + (c - 3) * kMaxL);   // smx, smy, sI are contiguous
#pragma unroll
			for (int r = 0; r < 4; ++r) {
				const int j0 = mfma_row(r, g), j1 = 16 + mfma_row(r, g);
				if (j0 < L) out[j0] = acc0[r];
				if (j1 < L) out[j1] = acc1[r];
			}
		}
	}
	env_sync();
	// ---- generalised bias
	{
		const real sfx = ws.sfs[0][j], sfy = ws.sfs[1][j], sfn = ws.sfs[2][j];
		const real bl = sfn - px * sfy + py * sfx;
		if (mine) {
			ws.sm[j] = subm;
			ws.b[j + 2] = bl;
			if (j == 0) { ws.b[0] = sfx; ws.b[1] = sfy; }
		}
	}
	env_sync();
	PROF_ADD(ws, kProfP4);
}

#if defined(DTRL_PROFILE)
// constraint-row bucket of the per-bucket counters (kProfFsubR0, kProfR0, kProfT0): 0 rows, 1-6, 7-12, 13-18, 19+
__device__ __forceinline__ int prof_row_bucket(int R) { return R == 0 ? 0 : (R <= 6 ? 1 : (R <= 12 ? 2 : (R <= 18 ? 3 : 4))); }
#endif
// Which instances run the slot-order passes: those compiled for two waves per SIMD (256 VGPRs). An instance compiled for three (168 VGPRs: the fp32 library's raptor)
// keeps the row-order sequences: in slot order its substep loop holds 135 scratch instructions against 8, and the fp32 leg of configs[2] loses 11 %
// (docs/EXPERIMENTS.md 38, profiles/contact_solve.txt 2).
// WavesPerEu<Topo> is the register budget the unit gives the instance (dtrl_frame_entry.h). It is only declared here and looked up when FastPath<Topo> is instantiated:
// a unit that instantiates the fast path without defining it does not compile.
template <class Topo> struct WavesPerEu;
template <class Topo> struct PgsSlotOrder { static constexpr bool value = WavesPerEu<Topo>::value <= 2; };
template <class Topo>
struct FastPath {
	static constexpr int D = Topo::L + 2;
	static constexpr int NP = pts_per_lane(Topo::L);   // contact sample points per lane
	static __device__ void substep(WSFast& ws, const DevModel& gm, const GroundRec& g, real h, bool kin_valid)
	{
		const int lane = static_cast<int>(threadIdx.x);
#if defined(DTRL_PROFILE)
		const unsigned long long prof_sub_t0 = __builtin_readcyclecounter();
#endif
		if (!kin_valid) { PROF_T0(); kin_dyn_terms_fast<Topo>(ws); PROF_ADD(ws, kProfFK); }
		// constraint rows first, factorisation second: the two are independent (both read the kinematics only), and in this order neither the
		// 23 doubles of the lane's matrix row are live across the contact pass (and its out-of-line calls) nor the sample points across the elimination.
		// The post-step contact pass of the previous env-step (contacts() below) ran at this very configuration and left its constraint
		// row list in LDS: the first substep of an env-step takes it over instead of sampling the heightfield again
		const int rows_ready = kin_valid ? ws.n_pts_active : -1;   // wave-uniform
		if (rows_ready >= 0) {
			if (lane == 0) { ws.R = rows_ready; ws.n_pts_active = -1; }
			env_sync();
		} else {
			ContactPts cp;
			{ PROF_T0(); cp = eval_points<Topo::L, false>(ws, gm, g); PROF_ADD(ws, kProfDetect); }   // the per-link contact flags are the post-step pass's business (contacts() below)
			{ PROF_T0(); build_rows_fast<NP>(ws, gm, cp, h); PROF_ADD(ws, kProfRows); }
		}
		real hrow[D];
		{ PROF_T0(); mass_row<D>(ws, hrow); PROF_ADD(ws, kProfMass); }
		real dinv;
		{ PROF_T0(); dinv = factorize_regs<Topo>(ws, hrow); PROF_ADD(ws, kProfFact); }
		// the row count, the cache's and the warm-start switch: read ONCE, here, and handed down to warm_match_fast(), build_delassus_fast() and pgs_solve_fast() as
		// wave-uniform values
		const int R = __builtin_amdgcn_readfirstlane(ws.R), Rp = __builtin_amdgcn_readfirstlane(ws.st.ws_R);
		const bool warm = __builtin_amdgcn_readfirstlane(ws.M.warm_start) != 0;
		{ PROF_T0(); warm_match_fast(ws, R, Rp, warm); PROF_ADD(ws, kProfRows); }
		if (lane == 0) ws.cost += 8 + R;
		{
			PROF_T0();
			// J_r[lane] from wave-uniform row descriptors and the lane's own joint position (registers): same value as row_jac()
			const bool hinge = lane >= 2 && lane < D;
			const real mypx = hinge ? ws.px[lane - 2] : 0.0, mypy = hinge ? ws.py[lane - 2] : 0.0;
			const uint32_t mysub = hinge ? ws.M.sub_mask[lane - 2] : 0u;
			real rhs0 = (lane < D) ? (ws.st.tau[lane] - ws.b[lane]) : 0.0;
			if (__builtin_expect(ws.st.pert_on != 0, 0)) { if (lane < D) rhs0 += perturb_gen_force(ws, lane); }
			if (R < 1) {
				// airborne, one right-hand side: the lane = DoF broadcast chain in registers is cheaper than the row form
				// (under a second test of R: with `R == 0` alone the compiler allocates the substep loop differently and spills in it)
				if (0 <= R) {
					const real z = usolve_regs<D>(hrow, rhs0);
					if (lane < D) ws.Z[0][lane] = z;
				}
			} else {
				// the R + 1 right-hand sides into Z unsolved (lane = DoF), then solved in place with lane = row.
				// The row descriptors do not come through LDS one row at a time (kind and link, wait, link2, wait, dx / dy / x / y, wait -- three to four
				// dependent trips per row in a loop that is neither unrolled nor pipelined): lane r loads ITS row's descriptor -- one batch, one wait; lane-indexed,
				// unconditional and clamped like the batched PD set-up of controller_update() -- and row r's is broadcast from lane r (v_readlane with a wave-uniform
				// lane index: the values arrive in SGPRs), so the kind of the row is wave-uniform as before and the operations are row_jac()'s, DoF = lane, on the same values.
				// (Building row r's entries on lane r inside usolve_rows() instead was measured and lost: docs/EXPERIMENTS.md 33.)
				{
					const int ol = opaque_lane();   // (the seven lane-indexed addresses are formed here, not kept across the substep loop as loop invariants)
					const int rc = ol < R ? ol : 0; // (lanes >= R: row 0 exists, the values are not used)
					const int kind_l = ws.row_kind[rc], link_l = ws.row_link[rc], link2_l = ws.row_link2[rc];
					const real dx_l = ws.row_dx[rc], dy_l = ws.row_dy[rc], x_l = ws.row_x[rc], y_l = ws.row_y[rc];
					for (int r = 0; r < R; ++r) {
						const int kind = __builtin_amdgcn_readlane(kind_l, r), link = __builtin_amdgcn_readlane(link_l, r);
						const real dx = bcast(dx_l, r);
						real v;
						if (kind == 0) v = (lane == link + 2) ? dx : 0.0;
						else {
							const real dy = bcast(dy_l, r), x = bcast(x_l, r), y = bcast(y_l, r);
							const int link2 = __builtin_amdgcn_readlane(link2_l, r);
							const int on = static_cast<int>((mysub >> link) & 1u) - (link2 < 0 ? 0 : static_cast<int>((mysub >> link2) & 1u));
							const real jr = dx * (-(y - mypy)) + dy * (x - mypx);
							v = on == 0 ? 0.0 : (on > 0 ? jr : -jr);
							v = (lane == 0) ? (link2 < 0 ? dx : 0.0) : v;
							v = (lane == 1) ? (link2 < 0 ? dy : 0.0) : v;
						}
						if (lane < D) ws.Z[r][lane] = v;
					}
					if (lane < D) ws.Z[R][lane] = rhs0;
				}
				env_sync();
				usolve_rows<Topo>(ws, R);
			}
			if (lane < D) ws.dinv[lane] = dinv;   // the Delassus product reads 1/d per DoF from LDS
			env_sync();
			PROF_ADD(ws, kProfFsub);
#if defined(DTRL_PROFILE)
			PROF_ADD(ws, kProfFsubR0 + prof_row_bucket(R));
#endif
		}
		if (R > 0) {
			real w;
			{ PROF_T0(); w = build_delassus_fast<D>(ws, h, dinv, R); PROF_ADD(ws, kProfDelassus); }
			{ PROF_T0(); pgs_solve_fast<Topo::kPgsRegRows, PgsSlotOrder<Topo>::value>(ws, R, warm, w); PROF_ADD(ws, kProfPgs); }
		}
		{
			PROF_T0();
			real u = 0;
			if (lane < D) {
				real s = h * ws.Z[R][lane];
				for (int r = 0; r < R; ++r) s = fmadd(ws.Z[r][lane], ws.st.ws_lam[r], s);
				u = s * dinv;
			}
			u = utsolve_regs<D>(hrow, u);
			if (lane < D) { const real v = clamp_turn_rate(ws.st.qd[lane] + u, lane, h); ws.st.qd[lane] = v; ws.st.q[lane] += h * v; }
			env_sync();
			PROF_ADD(ws, kProfFinish);
		}
#if defined(DTRL_PROFILE)
		if (threadIdx.x == 0) { ws.prof[kProfRowsSum] += R; ws.prof[kProfSubsteps] += 1; const int bk = prof_row_bucket(R); ws.prof[kProfR0 + bk] += 1; ws.prof[kProfT0 + bk] += __builtin_readcyclecounter() - prof_sub_t0; }
#endif
	}
	static __device__ void kinematics(WSFast& ws) { kin_dyn_terms_fast<Topo>(ws); }   // env_step()'s post-step evaluation
	static __device__ void pd_solve(WSFast& ws, real dt)
	{
		const int lane = static_cast<int>(threadIdx.x);
		real hrow[D];
		mass_row<D>(ws, hrow);   // composite inertias come from kin_dyn_terms() in env_step
		const real add = (lane < D) ? dt * ws.kdm[lane] : 0.0;
#pragma unroll
		for (int k = 0; k < D; ++k) if (lane == k) hrow[k] += add;
		const real dinv = factorize_regs<Topo>(ws, hrow);
		real z = (lane < D) ? ws.u[lane] : 0.0;
		z = usolve_regs<D>(hrow, z);
		real u = z * dinv;
		u = utsolve_regs<D>(hrow, u);
		env_sync();
		if (lane < D) ws.u[lane] = u;
		if (lane == 0) ws.R = 0;
		env_sync();
	}
	// cContactManager::Update at the post-step configuration: the controller needs the per-link flags; the same pass builds the row list of
	// the next env-step's first substep (same q, same heightfield window within a launch)
	static __device__ void contacts(WSFast& ws, const DevModel& gm, const GroundRec& g, real h)
	{
		const ContactPts cp = eval_points<Topo::L, true>(ws, gm, g);
		contact_bits_fast<NP>(ws, cp.f0, cp.f1, cp.f2);
		build_rows_fast<NP>(ws, gm, cp, h);
		if (threadIdx.x == 0) ws.n_pts_active = ws.R;
		env_sync();
	}
};

}  // namespace dtrl
#endif  // __HIP_DEVICE_COMPILE__
