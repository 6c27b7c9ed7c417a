// dtrl_topo.h -- skeleton topologies the register fast path is compiled for (dtrl_kernel_fast.h).
// The fast path eliminates the joint-space inertia matrix leaf-to-root; with the parent table known at compile time the updates that
// are structurally zero (DoF pairs that are not on one root->leaf path) are simply not emitted. A character whose parent table
// matches none of these runs on the generic LDS-phase kernel (same results, slower).
// Parent tables: data/characters/dog.txt and goat.txt (same skeleton), raptor.txt of the reference.
#pragma once
#include <cstdint>
#include "dtrl_types.h"

namespace dtrl {

struct TopoDog {
	static constexpr int kId = 1;
	static constexpr int L = 21;
	// constraint rows the projected Gauss-Seidel keeps in registers (dtrl_kernel_fast.h pgs_solve_fast). A launch lasts as long as its slowest env, and the slowest
	// envs of a frame are characters lying on 13-24 rows per substep: with every row count on the unrolled path the dog's 2048-env launch went 4.71 -> 4.45 ms
	// (16.7 -> 17.8 M env-steps/s), with nested row sequences -> 4.33 ms (18.1 M), with 20 register rows + the tail rows from LDS -> 4.26 ms (18.4 M): same-box A/Bs in
	// profiles/r04_pgs_rows_ab.txt
	// Round 5, with the per-pass row steps: 17.22 M at 24 (= kMaxRows: no substep leaves the unrolled path) against 16.9 M at 20, 14.4 M at 20 + plain loop: profiles/r05_pgs_rows_ab.txt
	static constexpr int kPgsRegRows = 24;
	static_assert(kPgsRegRows <= kMaxRows, "more register rows than constraint rows");
	static constexpr int parent(int l) { constexpr int p[L] = {-1, 0, 1, 2, 3, 4, 5, 6, 7, 0, 9, 10, 11, 5, 13, 14, 15, 0, 17, 18, 19}; return p[l]; }
};
struct TopoRaptor {
	static constexpr int kId = 2;
	static constexpr int L = 19;
	// the raptor's instance pays for the registers of 24 rows with spills: it keeps 16 and sends a substep with more rows through the plain loop (nested row sequences,
	// round 4: 18.65 M at 12, 18.88 M at 16, 18.82 M at 24; flat sequences had 18.4 / 18.1 / 17.2 M at 12 / 18 / 24: profiles/r04_pgs_rows_ab.txt)
	static constexpr int kPgsRegRows = 16;
	static_assert(kPgsRegRows <= kMaxRows, "more register rows than constraint rows");
	static constexpr int parent(int l) { constexpr int p[L] = {-1, 0, 1, 2, 3, 4, 0, 6, 7, 8, 9, 0, 11, 12, 13, 0, 15, 16, 17}; return p[l]; }
};

// link a is l or an ancestor of l
template <class T>
constexpr bool link_on_path(int a, int l)
{
	while (l >= 0) { if (l == a) return true; l = T::parent(l); }
	return false;
}
// entries of the longest root->link path (the link itself included): what the path loops of kin_dyn_terms_fast() run to (dog: 10, raptor: 6)
template <class T>
constexpr int topo_depth()
{
	int d = 0;
	for (int l = 0; l < T::L; ++l) { int n = 0; for (int a = l; a >= 0; a = T::parent(a)) ++n; d = n > d ? n : d; }
	return d;
}
// entry (j, k), j < k, of the joint-space inertia matrix is structurally non-zero during the leaf-first elimination. DoFs 0, 1 are the
// root translations: every hinge hangs below them (H(0,1) itself starts at zero but fills in as the hinges are eliminated);
// DoF d >= 2 is the hinge of link d - 2
template <class T>
constexpr bool dof_coupled(int j, int k)
{
	if (j < 2) return true;
	return link_on_path<T>(j - 2, k - 2);
}
template <class T>
inline bool topology_matches(const int32_t* parent, int L)
{
	if (L != T::L) return false;
	for (int l = 0; l < L; ++l) if (parent[l] != T::parent(l)) return false;
	return true;
}
// 0 = no compiled-in topology (generic kernel)
inline int match_topology(const int32_t* parent, int L)
{
	if (topology_matches<TopoDog>(parent, L)) return TopoDog::kId;
	if (topology_matches<TopoRaptor>(parent, L)) return TopoRaptor::kId;
	return 0;
}

}  // namespace dtrl
