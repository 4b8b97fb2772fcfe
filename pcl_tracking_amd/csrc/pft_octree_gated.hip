// pft_octree_gated.hip -- the change-detection instances of the single-workgroup builder and of the leaf gather
// (k_octree_build<true>, k_leaf_gather<true>: they return at once when PftDev::gate says nothing changed).  A translation
// unit of their own, so that the default instances in pft_octree.hip compile exactly as before.
#define PFT_OCTREE_GATED_TU
#include "pft_octree.hip"

template __global__ void k_octree_build<true>(PftParams, PftDev, uint32_t, int, int, int);
template __global__ void k_leaf_gather<true>(PftDev);
