"""The linearised octree of pcl_tracking_amd/csrc/pft_octree.hip / pft_octree_sorted.hip restated in plain numpy (test
infrastructure only).  Three independent pieces:

  linearise(depth, keys, ...)   the specified tree -- words, level starts, leaf order, jump table, header fields -- as a pure
                                integer function of the depth and the per-point keys in insertion order
  walk(words, lvl_start, ...)   decodes ANY tree from the root by following masks and bases, without assuming an order inside
                                a level, and asserts that it is well formed
  predict_variant(...)          the dispatch rule of k_octree_build / pftk_octree / the host's builder choice, as the code of
                                PftHeader::build_variant

Layout: levels contiguous and in Morton order (child index x << 2 | y << 1 | z, level-1 digit most significant); the children
of a node contiguous and ordered by child index; branch word = mask | child_base << 8 with child_base an absolute index into
words; leaf word = the leaf's start in leaf order; one sentinel word holds n.
"""
import numpy as np

TABLE_MAX_DEPTH = 10   # PFT_TABLE_MAX_DEPTH
JUMP_MAX_LEVEL = 4     # PFT_JUMP_MAX_LEVEL
BUILD_THREADS = 1024   # PFT_BUILD_THREADS
SORTED_BUILD_MIN = 18000  # PFT_SORTED_BUILD_MIN
MAX_CODE_DEPTH = 21    # 3 * 21 bits fit a 64-bit Morton code (the sorted builder's own limit)

STORE_REG4, STORE_REG8, STORE_REG14, STORE_HYBRID8, STORE_GLOB, STORE_SORTED = 1, 2, 3, 4, 5, 6
BIT_WORDS_LDS, BIT_TMP_LDS, BIT_LDS_ABANDONED, BIT_DENSE_TOP, BIT_RESCUE = 8, 16, 32, 64, 128


def jump_level(depth):
    return min(depth - 1, JUMP_MAX_LEVEL) if 4 <= depth <= TABLE_MAX_DEPTH else 0


def morton(keys, depth):
    """[n, 3] keys -> uint64 codes, digit of level l (1-based) at bits 3 * (depth - l)"""
    assert 0 < depth <= MAX_CODE_DEPTH
    k = np.asarray(keys, np.uint64).reshape(-1, 3)
    assert (k < (1 << depth)).all(), "key outside the depth's range"
    code = np.zeros(len(k), np.uint64)
    for b in range(depth):
        dig = (((k[:, 0] >> np.uint64(b)) & np.uint64(1)) << np.uint64(2)) | \
              (((k[:, 1] >> np.uint64(b)) & np.uint64(1)) << np.uint64(1)) | ((k[:, 2] >> np.uint64(b)) & np.uint64(1))
        code |= dig << np.uint64(3 * b)
    return code


def demorton(code, levels):
    """uint64 Morton prefixes of `levels` digits -> [m, 3] keys"""
    code = np.asarray(code, np.uint64)
    out = np.zeros((len(code), 3), np.uint64)
    for b in range(levels):
        dig = (code >> np.uint64(3 * b)) & np.uint64(7)
        out[:, 0] |= ((dig >> np.uint64(2)) & np.uint64(1)) << np.uint64(b)
        out[:, 1] |= ((dig >> np.uint64(1)) & np.uint64(1)) << np.uint64(b)
        out[:, 2] |= (dig & np.uint64(1)) << np.uint64(b)
    return out.astype(np.uint32)


def header_floats(depth, res, box_min, box_max):
    """margin_cells, inv_res, ominf exactly as the header tail forms them ("safety margin"): double IEEE operations in the
    same order, then one cast to float -> (uint32 bits, uint32 bits, uint32[3] bits)"""
    mn, mx = np.asarray(box_min, np.float64), np.asarray(box_max, np.float64)
    res = np.float64(res)
    maxabs = np.float64(0.0)
    for a in range(3):
        maxabs = max(maxabs, max(abs(mn[a]), abs(mx[a])))
    eta = maxabs * np.float64(1.1920928955078125e-07)
    s_top = res * np.float64(1 << (depth - 1 if depth > 0 else 0))
    E = np.float64(9.0) * eta + np.float64(40.0) * np.float64(5.9604644775390625e-08) * s_top
    mc = np.float64(2.0) * E / res + np.float64(1.0e-3)
    margin = np.float32(mc if mc < 0.25 else 1.0)
    inv_res = np.float32(np.float64(1.0) / res)
    return (int(np.array([margin]).view(np.uint32)[0]), int(np.array([inv_res]).view(np.uint32)[0]),
            mn.astype(np.float32).view(np.uint32).copy())


def linearise(depth, keys, res=None, box_min=None, box_max=None):
    keys = np.asarray(keys, np.uint32).reshape(-1, 3)
    n, D = len(keys), int(depth)
    assert n > 0 and D > 0
    code = morton(keys, D)
    order = np.argsort(code, kind="stable")  # insertion order inside a leaf
    sc = code[order]
    prefixes = [np.unique(sc >> np.uint64(3 * (D - l))) for l in range(D + 1)]  # sorted: Morton order inside a level
    lvl_start = np.zeros(D + 2, np.uint32)
    lvl_start[1:] = np.cumsum([len(p) for p in prefixes])
    n_words = int(lvl_start[D + 1]) + 1
    words = np.zeros(n_words, np.uint32)
    for l in range(D):
        par, ch = prefixes[l], prefixes[l + 1]
        owner = np.searchsorted(par, ch >> np.uint64(3))  # the children of a node are adjacent in the sorted child level
        mask = np.zeros(len(par), np.uint32)
        np.bitwise_or.at(mask, owner, (np.uint32(1) << (ch & np.uint64(7)).astype(np.uint32)))
        first = np.searchsorted(owner, np.arange(len(par)), side="left")
        words[lvl_start[l]:lvl_start[l + 1]] = mask | ((lvl_start[l + 1] + first).astype(np.uint32) << np.uint32(8))
    words[lvl_start[D]:lvl_start[D + 1]] = np.searchsorted(sc, prefixes[D], side="left")
    words[n_words - 1] = n
    J = jump_level(D)
    jump = np.zeros(1 << (3 * J) if J else 0, np.uint16)
    if J:
        c = demorton(prefixes[J], J).astype(np.int64)
        jump[c[:, 0] | (c[:, 1] << J) | (c[:, 2] << (2 * J))] = np.arange(1, len(c) + 1)
    t = dict(depth=D, n=n, words=words, lvl_start=lvl_start, leaf_start=int(lvl_start[D]), n_leaves=len(prefixes[D]),
             n_words=n_words, leaf_order=order.astype(np.uint32), jump=jump, jump_level=J,
             use_table=int(D <= TABLE_MAX_DEPTH))
    if res is not None:
        t["margin_cells_bits"], t["inv_res_bits"], t["ominf_bits"] = header_floats(D, res, box_min, box_max)
    return t


def walk(words, lvl_start, depth, leaf_order, n):
    """-> {leaf key (x, y, z): point indices in stored order}; AssertionError on a malformed tree"""
    words = np.asarray(words, np.uint32).astype(np.int64)
    lvl = np.asarray(lvl_start, np.int64)
    D = int(depth)
    assert len(lvl) >= D + 2 and lvl[0] == 0 and lvl[1] == 1, "the root level is not [0, 1)"
    n_words = int(lvl[D + 1]) + 1
    assert len(words) >= n_words, "words shorter than the level starts say"
    nodes, prefix = np.zeros(1, np.int64), np.zeros(1, np.uint64)
    lanes = np.arange(8, dtype=np.int64)
    for l in range(D):
        w = words[nodes]
        mask, base = w & 0xff, w >> 8
        assert (mask != 0).all(), "level %d: reached branch %d has an empty mask" % (l, nodes[np.argmin(mask != 0)])
        bits = (mask[:, None] >> lanes) & 1
        rank = np.cumsum(bits, axis=1) - bits
        sel = bits == 1
        child = (base[:, None] + rank)[sel]
        cpre = ((prefix[:, None] << np.uint64(3)) | lanes.astype(np.uint64))[sel]
        lo, hi = int(lvl[l + 1]), int(lvl[l + 2])
        srt = np.sort(child)
        ok = len(child) == hi - lo and (srt == np.arange(lo, hi)).all()
        if not ok:
            bad = np.setdiff1d(np.arange(lo, hi), child)
            dup = srt[1:][srt[1:] == srt[:-1]]
            raise AssertionError("level %d: children do not fill [%d, %d) exactly once (first unreached %s, first reached "
                                 "twice %s, outside %s)" % (l + 1, lo, hi, bad[:1], dup[:1], srt[(srt < lo) | (srt >= hi)][:1]))
        nodes, prefix = child, cpre
    o = np.argsort(nodes)  # leaf words in index order (their order in the level is not assumed)
    nodes, prefix = nodes[o], prefix[o]
    starts = np.concatenate([words[nodes], words[n_words - 1:n_words]])
    assert starts[-1] == n, "sentinel %d, not n = %d" % (starts[-1], n)
    assert (np.diff(starts) >= 0).all(), "leaf starts decrease at leaf word %d" % nodes[np.argmax(np.diff(starts) < 0)]
    assert starts[0] >= 0 and starts[-1] <= len(leaf_order)
    lo_ = np.asarray(leaf_order)
    keys = demorton(prefix, D)
    return {(int(k[0]), int(k[1]), int(k[2])): lo_[s:e].tolist() for k, s, e in zip(keys, starts[:-1], starts[1:])}


def key_groups(keys):
    """{key: ascending insertion indices} of the oracle's per-point keys: what a correct tree's walk returns"""
    out = {}
    for i, k in enumerate(np.asarray(keys).reshape(-1, 3).tolist()):
        out.setdefault((k[0], k[1], k[2]), []).append(i)
    return out


def descend(words, depth, key, from_node=0, from_level=0):
    """the integer descent of one key from a node -> (node reached, level reached): stops at an absent child"""
    node, l = int(from_node), int(from_level)
    while l < depth:
        sh = depth - 1 - l
        ch = (((int(key[0]) >> sh) & 1) << 2) | (((int(key[1]) >> sh) & 1) << 1) | ((int(key[2]) >> sh) & 1)
        w = int(words[node])
        if not (w >> ch) & 1:
            break
        node = (w >> 8) + bin(w & 0xff & ((1 << ch) - 1)).count("1")
        l += 1
    return node, l


_POPC = np.array([bin(i).count("1") for i in range(256)], np.int64)


def descend_all(words, levels, cells):
    """descend() for many keys at once: cells [m, 3] are coordinates at level `levels` (the full keys for levels = depth)
    -> (node reached, level reached) per cell; a descent stops at the first absent child"""
    words = np.asarray(words, np.uint32).astype(np.int64)
    c = np.asarray(cells, np.int64).reshape(-1, 3)
    node, lvl = np.zeros(len(c), np.int64), np.zeros(len(c), np.int64)
    alive = np.ones(len(c), bool)
    for l in range(levels):
        sh = levels - 1 - l
        ch = (((c[:, 0] >> sh) & 1) << 2) | (((c[:, 1] >> sh) & 1) << 1) | ((c[:, 2] >> sh) & 1)
        w = words[node]
        alive &= ((w >> ch) & 1) == 1
        nxt = (w >> 8) + _POPC[w & 0xff & ((1 << ch) - 1)]
        node = np.where(alive, nxt, node)
        lvl += alive
    return node, lvl


def sorted_npass(last_depth, forced=0):
    """radix passes the host gives the sorted builder: from the previous iteration's depth (0: unknown, all eight)"""
    npass = (3 * (last_depth + 1) + 7) // 8 if last_depth > 0 else 8
    if forced > 0:
        npass = forced
    return min(npass, 8)


def predict_variant(n, depth, n_words, lds_bytes, expected_points, forced_builder, leaf_indirect, last_depth=None,
                    forced_npass=0):
    """PftHeader::build_variant of the build of n points into a tree of `depth` levels and n_words words.
    expected_points / last_depth: the crop size and depth of the handle's previous build (0: none; last_depth defaults to
    depth, the second of two equal evaluations); forced_builder None | "single" | "sorted"; leaf_indirect: the handle
    follows leaf_order instead of copying the leaf records"""
    last_depth = depth if last_depth is None else last_depth
    use_sorted = expected_points > SORTED_BUILD_MIN
    if forced_builder == "single":
        use_sorted = False
    if forced_builder == "sorted":
        use_sorted = True
    rescue = False
    if use_sorted:
        npass = sorted_npass(last_depth, forced_npass)
        if 3 * depth <= 8 * npass:
            return STORE_SORTED | (npass << 10)
        rescue = True  # k_so_scan raises error bit 3, the rescue launch of k_octree_build rebuilds
    mode = 1 if rescue else (2 if leaf_indirect else (1 if expected_points <= 5000 else 0))
    if depth > TABLE_MAX_DEPTH or n > 18 * BUILD_THREADS:
        store = STORE_GLOB
    elif n <= 4 * BUILD_THREADS:
        store = STORE_REG4
    elif n <= 8 * BUILD_THREADS:
        store = STORE_REG8
    elif n <= 14 * BUILD_THREADS:
        store = STORE_REG14
    else:
        store = STORE_HYBRID8
    lds_words = lds_bytes // 4
    tmp_lds = n * 5 // 2 + 64 <= lds_words  # the carve: leaf scratch list beside the node words
    cap = lds_words - (((n + 3) & ~3) if tmp_lds else 0)
    v = store
    if cap >= 64:
        # every level's end + 2 must fit; the last and largest is the leaf level's: (n_words - 1) + 2
        if n_words + 1 <= cap:
            v |= BIT_WORDS_LDS | (BIT_TMP_LDS if tmp_lds else 0)
        else:
            v |= BIT_LDS_ABANDONED
    if jump_level(depth) > 0:
        v |= BIT_DENSE_TOP
    if rescue:
        v |= BIT_RESCUE
    return v | (mode << 8)


def decode_variant(v):
    return dict(store=v & 7, words_lds=bool(v & 8), tmp_lds=bool(v & 16), lds_abandoned=bool(v & 32), dense_top=bool(v & 64),
                rescue=bool(v & 128), leaf_mode=(v >> 8) & 3, npass=(v >> 10) & 15)
