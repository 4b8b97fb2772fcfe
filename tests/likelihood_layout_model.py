"""NumPy restatement of how k_likelihood (pcl_tracking_amd/csrc/pft_likelihood.hip) picks its LDS layout and its descent
from the tree's sizes, and the set of (layout, descent, jump table, leaf form) codes that rule can reach.

A code is "<layout>/<descent>[/nojump]/<direct|indirect>":
  layout   u16_leaf_starts (LEAF=1), u32_words (LEAF=0), branch_only (LEAF=2), hybrid (HybridWords)
  descent  fast, table_generic (centre tables, every level evaluated), no_table (depth > PFT_TABLE_MAX_DEPTH)
  nojump   the fast descent with the builder's jump table dropped to make the words fit
  direct / indirect  the INDIRECT instance (leaf records read through leaf_order)
"""
import numpy as np

PENALTY_BYTES = 256 * 8 * 4  # PFT_LIK_PENALTY=1: [256][8] float penalties by child mask
LUT_BYTES = 2048  # hue / saturation look-up tables
TABLE_MAX_DEPTH = 10  # PFT_TABLE_MAX_DEPTH
JUMP_MAX_LEVEL = 4  # PFT_JUMP_MAX_LEVEL

LAYOUTS = ("u16_leaf_starts", "u32_words", "branch_only", "hybrid")
DESCENTS = ("fast", "table_generic", "no_table")


def builder_jump_level(depth):
    """PftHeader::jump_level as both octree builders set it"""
    return min(depth - 1, JUMP_MAX_LEVEL) if 4 <= depth <= TABLE_MAX_DEPTH else 0


def predict(depth, n_crop, n_leaves, n_words, lds_bytes, allow_fast=True, margin_cells=0.0):
    """the kernel's choice for a tree of `depth` levels over `n_crop` points with `n_leaves` leaves and `n_words` node words
    (branch words + leaf starts + sentinel); allow_fast is False under PFT_GENERIC_DESCENT=1"""
    use_tab = 0 < depth <= TABLE_MAX_DEPTH
    per_axis = (2 << depth) if use_tab else 0
    fast = bool(allow_fast) and use_tab and np.float32(margin_cells) < np.float32(0.5)
    J = builder_jump_level(depth) if fast else 0
    used = PENALTY_BYTES + LUT_BYTES + 3 * per_axis * 4
    used = (used + 15) & ~15
    leaf_start = n_words - n_leaves - 1
    leaf16 = 0 < n_crop < 65536
    branch_bytes = leaf_start * 4 if leaf16 else n_words * 4
    leaf_bytes = (((n_leaves + 1) * 2 + 3) & ~3) if leaf16 else 0
    jump_bytes = (2 << (3 * J)) if J > 0 else 0
    fits_with_jump = used + jump_bytes + branch_bytes + leaf_bytes <= lds_bytes
    fits_without_jump = used + branch_bytes + leaf_bytes <= lds_bytes
    branch_only = use_tab and not fits_with_jump and leaf16 and used + jump_bytes + branch_bytes <= lds_bytes
    dropped = False
    if not fits_with_jump and fits_without_jump and not branch_only:
        dropped = J > 0
        J, jump_bytes = 0, 0
    used += jump_bytes
    words_in_lds = not branch_only and used + branch_bytes + leaf_bytes <= lds_bytes
    if branch_only:
        layout = "branch_only"
    elif words_in_lds:
        layout = "u16_leaf_starts" if leaf16 else "u32_words"
    else:
        layout = "hybrid"
    n_lds_words = 0 if (words_in_lds or branch_only) else min(n_words, (lds_bytes - used) // 4)
    descent = "fast" if fast else ("table_generic" if use_tab else "no_table")
    return dict(layout=layout, descent=descent, J=J, jump_dropped=dropped, n_lds_words=n_lds_words)


def code(layout, descent, jump_dropped, indirect):
    return "%s/%s%s/%s" % (layout, descent, "/nojump" if jump_dropped else "", "indirect" if indirect else "direct")


def code_of_record(rec):
    """the code of a decoded device record (tracker.decode_likelihood_layout)"""
    return code(rec["layout"], rec["descent"], rec["jump_dropped"], rec["indirect"])


def reachable_codes():
    """every code the rule can produce.  Not reachable (DESIGN.md "likelihood layouts"): branch_only without centre tables
    (the branch-only layout requires them), the jump table dropped in the branch-only or hybrid layouts (it is dropped only
    when the words then fit, which selects u16 / u32), and a dropped jump table without the fast descent (J is 0 then)."""
    out = set()
    for ind in (False, True):
        for layout in ("u16_leaf_starts", "u32_words", "hybrid"):
            for descent in DESCENTS:
                out.add(code(layout, descent, False, ind))
        for descent in ("fast", "table_generic"):
            out.add(code("branch_only", descent, False, ind))
        for layout in ("u16_leaf_starts", "u32_words"):
            out.add(code(layout, "fast", True, ind))
    return out
