"""The contract of the GPU BVH builders (v-img_amd/csrc/bvh_build.hip) restated in numpy: float32 where
the kernels are float32, every + - * / one float32 operation in the kernels' order (the library is built without
contraction and with a correctly rounded divide, so each expression has one result), integers where they use integers.
The kernels number nodes with atomic counters; nothing of that numbering reaches the arrays they emit, so the
restatement numbers nodes as it likes and emits the same layout: vimg_hip_build_lbvh / _ploc must give these bytes.
tests/test_bvh_build.py pins this file on its own, without a GPU.

Inputs are finite boxes with lo <= hi and no -0.0 coordinate (a minimum over +0 and -0 has no single answer here)."""
import numpy as np

F = np.float32
NONE = 0xFFFFFFFF
RADIUS, CUT = 12, 16384          # PLOC_R, kTopItems
TOP_BINS, TOP_SAH_LEVELS, LEAF_MAX = 32, 40, 8
ROUND_CAP = 4096


def half_area(lo, hi):
    """dx dy + dx dz + dy dz of boxes [..., 3] float32, summed left to right."""
    d = hi - lo
    return (d[..., 0] * d[..., 1] + d[..., 0] * d[..., 2]) + d[..., 1] * d[..., 2]


def _expand10(v):
    v = v.astype(np.uint32)
    v = (v * np.uint32(0x00010001)) & np.uint32(0xFF0000FF)
    v = (v * np.uint32(0x00000101)) & np.uint32(0x0F00F00F)
    v = (v * np.uint32(0x00000011)) & np.uint32(0xC30C30C3)
    v = (v * np.uint32(0x00000005)) & np.uint32(0x49249249)
    return v


def morton_codes(bounds6):
    """The 30-bit code of every primitive: 10 bits per axis of (c - lo) / (hi - lo) * 1024 clamped to 1023 over the
    bounds of the centres c = (lo + hi) * 0.5, 0 on an axis without extent; x takes the highest of each three bits."""
    b = np.asarray(bounds6, dtype=F).reshape(-1, 6)
    c = (b[:, :3] + b[:, 3:]) * F(0.5)
    lo, hi = c.min(0), c.max(0)
    code = np.zeros(len(b), np.uint32)
    for a in range(3):
        if hi[a] > lo[a]:
            t = (c[:, a] - lo[a]) / (hi[a] - lo[a])
        else:
            t = np.zeros(len(b), F)
        t = t * F(1024)
        t = np.where(t > F(1023), F(1023), np.where(t > F(0), t, F(0)))
        code |= _expand10(t.astype(np.uint32)) << np.uint32(2 - a)
    return code


def morton_keys(bounds6):
    """(keys, order): the 64-bit keys (code << 32 | primitive) in ascending order, and the primitives in that order."""
    code = morton_codes(bounds6)
    keys = (code.astype(np.uint64) << np.uint64(32)) | np.arange(len(code), dtype=np.uint64)
    keys = np.sort(keys)
    return keys, (keys & np.uint64(0xFFFFFFFF)).astype(np.uint32)


# ---- the reference layout ----------------------------------------------------------------------------------------
class Tree:
    """A binary tree over the sorted leaves.  ids: [0, n) the leaves in sorted order, n + i the internal node i with
    children left[i], right[i]; box [ids, 6]; nprims and as_leaf per id ("this subtree is emitted as ONE leaf")."""

    def __init__(self, n, ids):
        self.n = n
        self.left = np.full(ids, NONE, np.int64)
        self.right = np.full(ids, NONE, np.int64)
        self.box = np.zeros((n + ids, 6), F)
        self.nprims = np.ones(n + ids, np.int64)
        self.as_leaf = np.zeros(n + ids, bool)
        self.root = 0


def emit(tree, order):
    """(num_nodes, max_depth, nodes [num_nodes, 2] uint32, bb [2 num_nodes + 2, 3] float32, obj_indices [n] uint32):
    breadth-first numbering, the k-th node with children (in that order) owns nodes 1 + 2k and 2 + 2k, the boxes of a
    sibling pair at first_child side by side in rows 2 first_child + 2 .. + 5 {Lmin, Rmin, Lmax, Rmax}, the root's box
    in rows 0 and 2, rows 1 and 3 zero; a leaf is {first index into obj_indices, count}, leaves numbered in the same
    breadth-first order, a leaf of several primitives flattened depth first, left before right."""
    n = tree.n
    nodes = np.zeros((2 * n - 1, 2), np.uint32)
    bb = np.zeros((2 * (2 * n - 1) + 2, 3), F)
    obj = np.zeros(n, np.uint32)
    bb[0], bb[2] = tree.box[tree.root, :3], tree.box[tree.root, 3:]
    level, child_base, cursor, depth = [(tree.root, 0)], 1, 0, 0
    while level:
        depth += 1
        nxt = []
        for tid, out in level:
            if tid < n or tree.as_leaf[tid]:
                count = 1 if tid < n else int(tree.nprims[tid])
                nodes[out] = (cursor, count)
                stack = [tid]
                while stack:
                    r = stack.pop()
                    if r < n:
                        obj[cursor] = order[r]
                        cursor += 1
                    else:
                        stack.append(int(tree.right[r - n]))
                        stack.append(int(tree.left[r - n]))
                continue
            first = child_base
            child_base += 2
            nodes[out] = (first, 0)
            c0, c1 = int(tree.left[tid - n]), int(tree.right[tid - n])
            base = 2 * first + 2
            bb[base], bb[base + 1] = tree.box[c0, :3], tree.box[c1, :3]
            bb[base + 2], bb[base + 3] = tree.box[c0, 3:], tree.box[c1, 3:]
            nxt += [(c0, first), (c1, first + 1)]
        level = nxt
    assert cursor == n
    return child_base, depth, nodes[:child_base], bb[:2 * child_base + 2], obj


# ---- LBVH ----------------------------------------------------------------------------------------------------------
def radix_tree(keys):
    """Karras 2012 over sorted unique 64-bit keys: (left, right) of the n - 1 internal nodes, node 0 the root; a child
    c < n is the leaf at sorted position c, otherwise the internal node c - n."""
    k = [int(x) for x in keys]
    n = len(k)

    def delta(i, j):
        return -1 if j < 0 or j >= n else 64 - (k[i] ^ k[j]).bit_length()

    left, right = np.zeros(n - 1, np.int64), np.zeros(n - 1, np.int64)
    for i in range(n - 1):
        d = 1 if delta(i, i + 1) - delta(i, i - 1) >= 0 else -1
        dmin = delta(i, i - d)
        lmax = 2
        while delta(i, i + lmax * d) > dmin:
            lmax *= 2
        ln, t = 0, lmax // 2
        while t >= 1:
            if delta(i, i + (ln + t) * d) > dmin:
                ln += t
            t //= 2
        j = i + ln * d
        dnode = delta(i, j)
        s, t = 0, (ln + 1) // 2
        while True:
            if delta(i, i + (s + t) * d) > dnode:
                s += t
            if t == 1:
                break
            t = (t + 1) // 2
        gamma = i + s * d + min(d, 0)
        left[i] = gamma if min(i, j) == gamma else n + gamma
        right[i] = gamma + 1 if max(i, j) == gamma + 1 else n + gamma + 1
    return left, right


def _boxes_bottom_up(tree):
    """The box of every internal node: min / max of its children's."""
    n = tree.n
    stack = [(tree.root, False)]
    while stack:
        tid, done = stack.pop()
        if tid < n:
            continue
        c0, c1 = int(tree.left[tid - n]), int(tree.right[tid - n])
        if not done:
            stack += [(tid, True), (c0, False), (c1, False)]
            continue
        tree.box[tid, :3] = np.minimum(tree.box[c0, :3], tree.box[c1, :3])
        tree.box[tid, 3:] = np.maximum(tree.box[c0, 3:], tree.box[c1, 3:])
        tree.nprims[tid] = tree.nprims[c0] + tree.nprims[c1]


def lbvh(bounds6):
    """vimg_hip_build_lbvh: the radix tree over the sorted keys, one primitive per leaf, boxes by min / max."""
    b = np.ascontiguousarray(bounds6, dtype=F).reshape(-1, 6)
    n = len(b)
    keys, order = morton_keys(b)
    tree = Tree(n, max(n - 1, 0))
    tree.box[:n] = b[order]
    if n > 1:
        tree.left[:], tree.right[:] = radix_tree(keys)
        tree.root = n
        _boxes_bottom_up(tree)
    return emit(tree, order)


# ---- PLOC -----------------------------------------------------------------------------------------------------------
def nearest(box, radius):
    """For every cluster of the array (boxes [c, 6] in array order) the position of its partner: among the positions
    within `radius`, the pair (i, j) that is smallest in the order
        (half area of the union, lower position odd, distance |i - j|, lower position).
    The order is total on pairs and both ends compute the same key, so the smallest pair of the whole array is always
    mutual - a round always merges - and where the unions tie exactly (equal boxes at equal spacing) the even / odd
    term lets every second pair merge in one round instead of one pair at an end."""
    c = len(box)
    best = np.full(c, np.inf, F)
    bkey = np.full(c, np.iinfo(np.uint64).max, np.uint64)
    nn = np.arange(c)
    for d in range(1, min(radius, c - 1) + 1):
        lo = np.minimum(box[:-d, :3], box[d:, :3])
        hi = np.maximum(box[:-d, 3:], box[d:, 3:])
        sa = half_area(lo, hi)
        low = np.arange(c - d, dtype=np.uint64)
        key = ((low & np.uint64(1)) << np.uint64(62)) | (np.uint64(d) << np.uint64(31)) | low
        for mine, other in ((slice(0, c - d), low.astype(np.int64) + d), (slice(d, c), low.astype(np.int64))):
            take = (sa < best[mine]) | ((sa == best[mine]) & (key < bkey[mine]))
            best[mine] = np.where(take, sa, best[mine])
            bkey[mine] = np.where(take, key, bkey[mine])
            nn[mine] = np.where(take, other, nn[mine])
    return nn


def agglomerate(tree, cost, parent, firstpos, radius):
    """The clustering rounds over tree's leaves; fills the tree (nodes n .. 2n - 2) and the three records; returns
    (root id, rounds)."""
    n = tree.n
    cluster = np.arange(n)
    made, rounds = 0, 0
    while len(cluster) > 1:
        nn = nearest(tree.box[cluster], radius)
        i = np.arange(len(cluster))
        mutual = (nn != i) & (nn[nn] == i)
        lower = np.nonzero(mutual & (i < nn))[0]
        rounds += 1
        if len(lower) == 0:
            raise RuntimeError("build_ploc: a clustering round merged nothing")
        if rounds > ROUND_CAP:
            raise RuntimeError("build_ploc: the clustering rounds ran out")
        a, b = cluster[lower], cluster[nn[lower]]
        ids = n + made + np.arange(len(lower))
        made += len(lower)
        tree.left[ids - n], tree.right[ids - n] = a, b
        lo = np.minimum(tree.box[a, :3], tree.box[b, :3])
        hi = np.maximum(tree.box[a, 3:], tree.box[b, 3:])
        tree.box[ids, :3], tree.box[ids, 3:] = lo, hi
        area = half_area(lo, hi)
        np_ = tree.nprims[a] + tree.nprims[b]
        split = np.full(len(ids), 0.5, F)
        with np.errstate(all="ignore"):
            for ch in (a, b):
                ratio = np.where(area > F(0), half_area(tree.box[ch, :3], tree.box[ch, 3:]) / area, F(1)).astype(F)
                split = split + ratio * cost[ch]
        leaf = np_.astype(F)
        ends = (np_ <= LEAF_MAX) & (leaf <= split)
        tree.nprims[ids], tree.as_leaf[ids] = np_, ends
        cost[ids] = np.where(ends, leaf, split)
        parent[a], parent[b] = ids, ids
        firstpos[ids] = np.minimum(firstpos[a], firstpos[b])
        merged = cluster.copy()
        merged[lower] = ids
        cluster = merged[~(mutual & (i > nn))]
    return int(cluster[0]), rounds


def cut_of(tree, parent, firstpos, cut):
    """The ids of the cut, ordered by first sorted position: keys are the half-area bits of the agglomeration's nodes
    with more than 8 primitives (0 for the others), the threshold the min(cut - 1, n - 1)-th largest key (1 at least),
    a node at or above it is opened, the cut is the closed nodes (leaves among them) under opened parents."""
    n = tree.n
    ids = np.arange(n, 2 * n - 1)
    key = np.where(tree.nprims[ids] > LEAF_MAX, half_area(tree.box[ids, :3], tree.box[ids, 3:]).view(np.uint32), 0).astype(np.uint32)
    opened = min(cut - 1, n - 1)
    tau = max(int(np.sort(key)[::-1][opened - 1]), 1)
    is_open = np.zeros(2 * n - 1, bool)
    is_open[ids] = key >= tau
    every = np.arange(2 * n - 1)
    has_parent = parent[every] != NONE
    member = has_parent & ~is_open
    member[has_parent] &= is_open[parent[every[has_parent]]]
    members = every[member]
    return members[np.argsort(firstpos[members], kind="stable")]


def _top_split(lo, hi, prims):
    """One node of the rebuilt top over items (boxes lo, hi [m, 3], primitives [m]): the mask of the items that go
    left, or None for "split at the median".  32 bins per axis over the bounds of the centres, the 31 splits of every
    axis with extent priced half_area(l) * float(prims_l) + half_area(r) * float(prims_r), the minimum over
    (cost bits, axis * 64 + split)."""
    c = F(0.5) * (lo + hi)
    cl, ch = c.min(0), c.max(0)
    best, best_mask = None, None
    for a in range(3):
        if not ch[a] > cl[a]:
            continue
        with np.errstate(all="ignore"):
            scale = F(TOP_BINS) / (ch[a] - cl[a])
            x = (c[:, a] - cl[a]) * scale
        x = np.where(x == x, x, F(0))
        bins = np.clip(x, 0, TOP_BINS - 1).astype(np.int64)           # (the kernel truncates, then clamps: the same)
        blo = np.full((TOP_BINS, 3), 3.4e38, F)
        bhi = np.full((TOP_BINS, 3), -3.4e38, F)
        np.minimum.at(blo, bins, lo)
        np.maximum.at(bhi, bins, hi)
        items = np.bincount(bins, minlength=TOP_BINS)
        pr = np.bincount(bins, weights=prims, minlength=TOP_BINS).astype(np.int64)
        l_lo, l_hi = np.minimum.accumulate(blo, 0)[:-1], np.maximum.accumulate(bhi, 0)[:-1]
        r_lo, r_hi = np.minimum.accumulate(blo[::-1], 0)[::-1][1:], np.maximum.accumulate(bhi[::-1], 0)[::-1][1:]
        li, lp = np.cumsum(items)[:-1], np.cumsum(pr)[:-1]
        ri, rp = items.sum() - li, pr.sum() - lp
        with np.errstate(all="ignore"):
            cost = half_area(l_lo, l_hi) * lp.astype(F) + half_area(r_lo, r_hi) * rp.astype(F)
        for s in np.nonzero((li > 0) & (ri > 0))[0]:
            k = (int(cost[s].view(np.uint32)) << 32) | (a * 64 + int(s))
            if best is None or k < best:
                best, best_mask = k, bins <= s
    return best_mask


def rebuild_top(tree, members):
    """The binned-SAH tree over the cut, top-down, a level at a time; new nodes from id 2n - 1.  Returns its root."""
    n = tree.n
    grow = len(members)                                                      # (fewer nodes than subtrees in the cut)
    tree.left = np.concatenate([tree.left, np.full(grow, NONE, np.int64)])
    tree.right = np.concatenate([tree.right, np.full(grow, NONE, np.int64)])
    tree.box = np.concatenate([tree.box, np.zeros((grow, 6), F)])
    tree.nprims = np.concatenate([tree.nprims, np.zeros(grow, np.int64)])
    tree.as_leaf = np.concatenate([tree.as_leaf, np.zeros(grow, bool)])
    nxt = 2 * n - 1
    root = nxt
    nxt += 1
    jobs, level = [(np.asarray(members), root)], 0
    while jobs:
        new_jobs = []
        for items, node in jobs:
            lo, hi, prims = tree.box[items, :3], tree.box[items, 3:], tree.nprims[items]
            tree.box[node, :3], tree.box[node, 3:] = lo.min(0), hi.max(0)
            tree.nprims[node] = prims.sum()
            mask = _top_split(lo, hi, prims) if level < TOP_SAH_LEVELS and len(items) > 2 else None
            if mask is None:
                mask = np.arange(len(items)) < len(items) // 2
            kids = []
            for side in (items[mask], items[~mask]):
                if len(side) == 1:
                    kids.append(int(side[0]))
                else:
                    kids.append(nxt)
                    new_jobs.append((side, nxt))
                    nxt += 1
            tree.left[node - n], tree.right[node - n] = kids
        jobs, level = new_jobs, level + 1
    return root


def ploc_tree(bounds6, radius=RADIUS, cut=CUT, top=True):
    """The PLOC build up to its tree: (tree, order, rounds, members of the cut or None when the top was not rebuilt)."""
    b = np.ascontiguousarray(bounds6, dtype=F).reshape(-1, 6)
    n = len(b)
    _, order = morton_keys(b)
    tree = Tree(n, max(n - 1, 0))
    tree.box[:n] = b[order]
    cost = np.ones(2 * n - 1, F)
    parent = np.full(2 * n - 1, NONE, np.int64)
    firstpos = np.arange(2 * n - 1)
    tree.root, rounds = agglomerate(tree, cost, parent, firstpos, max(1, int(radius)))
    members = None
    if top and n > 16:
        members = cut_of(tree, parent, firstpos, max(4, int(cut)))
        if len(members) >= 3:
            tree.root = rebuild_top(tree, members)
        else:
            members = None
    return tree, order, rounds, members


def ploc(bounds6, radius=RADIUS, cut=CUT, top=True):
    """vimg_hip_build_ploc (radius: VIMG_PLOC_R, cut: VIMG_PLOC_TOP, top=False: VIMG_PLOC_NO_TOP): the arrays of
    `emit`, then the number of clustering rounds."""
    tree, order, rounds, _ = ploc_tree(bounds6, radius, cut, top)
    return emit(tree, order) + (rounds,)
