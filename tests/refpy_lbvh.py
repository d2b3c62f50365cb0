"""Host restatement of the beam BVH's hierarchy kernels and a validator of built trees (test
infrastructure, next to refpy.py).

Written from the kernels' comments (bre_build.hip k_karras / k_refit / k_single, bre_roots.hip
k_collapse4, the record layouts of bre_device.h) and Karras 2012, "Maximizing Parallelism in the
Construction of BVHs, Octrees, and k-d Trees".  Plain numpy: every node is computed at once, every
loop has a fixed bound, and nothing here indexes outside an array: what the kernel would write out
of range on a malformed input is reported in `problems` instead.

Conventions (bre_device.h): a child >= 0 is an interior node, a child < 0 is leaf cluster ~child,
EMPTY_CHILD is no child; the root is node 0 and its parent is -1; a single leaf gives one node with
child = (~0, EMPTY_CHILD).  Leaf i's key is keys[i * leaf_size], compared from bit key_lo up; equal
keys are told apart by 64 + clz32(i ^ j).  All box comparisons are bit for bit (min and max do not
round).
"""
import numpy as np

EMPTY_CHILD = -(2 ** 31)
UNWRITTEN = -2  # a parent / leaf_parent word no node wrote (device memory would hold a stale value)
STACK_DEPTH = 128  # kStackDepth
MAX_DEPTH = 96  # what validate() allows, against kStackDepth
FLT_MAX = np.float32(3.4028234663852886e38)

NODE = np.dtype([("lo", "<f4", (2, 3)), ("hi", "<f4", (2, 3)), ("child", "<i4", (2,)), ("parent", "<i4"),
                 ("nleaf", "<i4")])
NODE4 = np.dtype([("lo", "<f4", (3, 4)), ("hi", "<f4", (3, 4)), ("child", "<i4", (4,)), ("pad", "<i4", (4,))])
assert NODE.itemsize == 64 and NODE4.itemsize == 128
_ITER = 72  # bound of every doubling / halving loop: more than the bits of any index


def _bit_length(x):
    x = np.asarray(x, np.uint64).copy()
    n = np.zeros(x.shape, np.int64)
    for s in (32, 16, 8, 4, 2, 1):
        hi = x >> np.uint64(s)
        m = hi != 0
        n += np.where(m, s, 0)
        x = np.where(m, hi, x)
    return n + (x != 0)


def clz64(x):
    return 64 - _bit_length(x)


def clz32(x):
    return 32 - _bit_length(np.asarray(x, np.uint64) & np.uint64(0xFFFFFFFF))


def leaf_keys(keys, leaf_size, key_lo):
    keys = np.ascontiguousarray(keys, np.uint64)
    return keys[::leaf_size] >> np.uint64(key_lo)


def _delta(lk, i, j):
    """Common-prefix length of leaves i and j (ldelta): -1 for j outside the leaves."""
    nleaf = lk.shape[0]
    ok = (j >= 0) & (j < nleaf)
    jj = np.where(ok, j, 0)
    x = lk[i] ^ lk[jj]
    d = np.where(x == 0, 64 + clz32((i ^ jj).astype(np.uint64)), clz64(x))
    return np.where(ok, d, -1)


def karras(keys, leaf_size=1, key_lo=0):
    """The topology k_karras (k_single for one leaf) builds over `keys`: a dict of child [nnodes, 2],
    parent [nnodes], nleaf_below [nnodes], leaf_parent [nleaf] (int32) and `problems`, the writes the
    kernel would have made outside its arrays (empty for a monotone key sequence)."""
    lk = leaf_keys(keys, leaf_size, key_lo)
    nleaf = lk.shape[0]
    assert nleaf >= 1
    if nleaf == 1:
        return {"child": np.array([[~0, EMPTY_CHILD]], np.int32), "parent": np.array([-1], np.int32),
                "nleaf_below": np.array([1], np.int32), "leaf_parent": np.array([0], np.int32), "problems": []}
    nn = nleaf - 1
    problems = []
    i = np.arange(nn, dtype=np.int64)
    d = np.where(_delta(lk, i, i + 1) - _delta(lk, i, i - 1) >= 0, 1, -1).astype(np.int64)
    dmin = _delta(lk, i, i - d)
    lmax = np.full(nn, 2, np.int64)
    for _ in range(_ITER):
        grow = _delta(lk, i, i + lmax * d) > dmin
        if not grow.any():
            break
        lmax = np.where(grow, lmax << 1, lmax)
    else:
        problems.append("the range doubling did not end")
    ln = np.zeros(nn, np.int64)
    t = lmax >> 1
    for _ in range(_ITER):
        if not (t >= 1).any():
            break
        take = (t >= 1) & (_delta(lk, i, i + (ln + t) * d) > dmin)
        ln = np.where(take, ln + t, ln)
        t = t >> 1
    j = i + ln * d
    dnode = _delta(lk, i, j)
    s = np.zeros(nn, np.int64)
    t = ln.copy()
    active = np.ones(nn, bool)
    for _ in range(_ITER):  # do { t = (t + 1) >> 1; ... } while (t > 1)
        if not active.any():
            break
        t = np.where(active, (t + 1) >> 1, t)
        take = active & (_delta(lk, i, i + (s + t) * d) > dnode)
        s = np.where(take, s + t, s)
        active &= t > 1
    gamma = i + s * d + np.minimum(d, 0)
    lo, hi = np.minimum(i, j), np.maximum(i, j)
    left_leaf, right_leaf = lo == gamma, hi == gamma + 1
    child = np.empty((nn, 2), np.int64)
    child[:, 0] = np.where(left_leaf, ~gamma, gamma)
    child[:, 1] = np.where(right_leaf, ~(gamma + 1), gamma + 1)
    parent = np.full(nn, UNWRITTEN, np.int64)
    leaf_parent = np.full(nleaf, UNWRITTEN, np.int64)
    for k in np.nonzero((gamma < 0) | (gamma > nleaf - 2))[0]:
        problems.append(f"node {k}: split index {gamma[k]} outside [0, {nleaf - 2}]")
    for side, is_leaf, tgt in ((0, left_leaf, gamma), (1, right_leaf, gamma + 1)):
        ok_leaf = is_leaf & (tgt >= 0) & (tgt < nleaf)
        ok_node = ~is_leaf & (tgt >= 0) & (tgt < nn)
        leaf_parent[tgt[ok_leaf]] = i[ok_leaf]
        parent[tgt[ok_node]] = i[ok_node]
        for k in np.nonzero(is_leaf & ~ok_leaf)[0]:
            problems.append(f"node {k}: leaf_parent[{tgt[k]}] written outside the {nleaf} leaves")
        for k in np.nonzero(~is_leaf & ~ok_node)[0]:
            what = "one record past the node array" if tgt[k] == nn else "outside the node array"
            problems.append(f"node {k}: child {side} is interior node {tgt[k]}: nodes[{tgt[k]}].parent written {what}"
                            f" ({nn} nodes)")
    parent[0] = -1
    return {"child": child.astype(np.int32), "parent": parent.astype(np.int32),
            "nleaf_below": (hi - lo + 1).astype(np.int32), "leaf_parent": leaf_parent.astype(np.int32),
            "problems": problems}


def leaf_boxes(boxes, leaf_size):
    """Per leaf cluster of `leaf_size` consecutive member boxes [m, 6] (lo xyz, hi xyz): the union
    (leaf_box; the last leaf may be ragged)."""
    boxes = np.ascontiguousarray(boxes, np.float32).reshape(-1, 6)
    m = boxes.shape[0]
    nleaf = (m + leaf_size - 1) // leaf_size
    pad = np.empty((nleaf * leaf_size, 6), np.float32)
    pad[:, :3], pad[:, 3:] = FLT_MAX, -FLT_MAX
    pad[:m] = boxes
    pad = pad.reshape(nleaf, leaf_size, 6)
    return np.concatenate([pad[:, :, :3].min(axis=1), pad[:, :, 3:].max(axis=1)], axis=1)


def _depths(child, cap):
    """Depth of every interior node by a level-wise sweep from node 0 (at most `cap` levels); -1:
    not reached."""
    nn = child.shape[0]
    depth = np.full(nn, -1, np.int64)
    level = np.array([0], np.int64)
    for dep in range(cap):
        level = level[depth[level] < 0]
        if level.size == 0:
            break
        depth[level] = dep
        c = child[level].ravel().astype(np.int64)
        level = np.unique(c[(c >= 0) & (c < nn)])
    return depth


def refit(child, lboxes):
    """k_refit / k_single: each node's two child boxes, the union of the leaf boxes below the child,
    carried bottom-up.  Returns lo [nnodes, 2, 3], hi [nnodes, 2, 3].  Needs a valid topology."""
    child = np.asarray(child, np.int64)
    lboxes = np.ascontiguousarray(lboxes, np.float32).reshape(-1, 6)
    nn = child.shape[0]
    lo = np.empty((nn, 2, 3), np.float32)
    hi = np.empty((nn, 2, 3), np.float32)
    lo[:], hi[:] = FLT_MAX, -FLT_MAX  # an empty child's box (k_single)
    depth = _depths(child, nn + 1)
    assert (depth >= 0).all(), "refit: a node is not reachable from the root"
    for dep in range(int(depth.max()), -1, -1):
        idx = np.nonzero(depth == dep)[0]
        for s in (0, 1):
            c = child[idx, s]
            lf = (c < 0) & (c != EMPTY_CHILD)
            lo[idx[lf], s] = lboxes[~c[lf], :3]
            hi[idx[lf], s] = lboxes[~c[lf], 3:]
            it = c >= 0
            lo[idx[it], s] = np.minimum(lo[c[it], 0], lo[c[it], 1])
            hi[idx[it], s] = np.maximum(hi[c[it], 0], hi[c[it], 1])
    return lo, hi


def make_nodes(topo, lboxes):
    """The Node records of a karras() topology over the leaf boxes."""
    nodes = np.zeros(topo["child"].shape[0], NODE)
    nodes["child"], nodes["parent"], nodes["nleaf"] = topo["child"], topo["parent"], topo["nleaf_below"]
    nodes["lo"], nodes["hi"] = refit(topo["child"], lboxes)
    return nodes


def build(keys, boxes, leaf_size=1, key_lo=0):
    """karras + refit + collapse4 of sorted keys and their member boxes: (nodes, leaf_parent, nodes4)."""
    topo = karras(keys, leaf_size, key_lo)
    assert not topo["problems"], topo["problems"][:3]
    nodes = make_nodes(topo, leaf_boxes(boxes, leaf_size))
    return nodes, topo["leaf_parent"], collapse4(nodes)


def collapse4(nodes):
    """k_collapse4: record i holds binary node i's grandchildren left to right (a leaf child stands
    for itself, an empty child is skipped); unused slots are EMPTY_CHILD with zero boxes, pad is zero."""
    nn = nodes.shape[0]
    out = np.zeros(nn, NODE4)
    out["child"] = EMPTY_CHILD
    child, lo, hi = nodes["child"], nodes["lo"], nodes["hi"]
    for i in range(nn):
        k = 0
        for c in (0, 1):
            ch = int(child[i, c])
            if ch == EMPTY_CHILD:
                continue
            if ch >= 0:
                src = [(ch, g) for g in (0, 1) if child[ch, g] != EMPTY_CHILD]
            else:
                src = [(i, c)]
            for (n, g) in src:
                out["lo"][i, :, k] = lo[n, g]
                out["hi"][i, :, k] = hi[n, g]
                out["child"][i, k] = child[n, g]
                k += 1
    return out


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _range_min_tables(lboxes):
    """Sparse tables of the leaf boxes: level k holds the union of 2^k consecutive leaves."""
    lo, hi = [lboxes[:, :3]], [lboxes[:, 3:]]
    n, w = lboxes.shape[0], 1
    while 2 * w <= n:
        lo.append(np.minimum(lo[-1][:-w], lo[-1][w:]))
        hi.append(np.maximum(hi[-1][:-w], hi[-1][w:]))
        w *= 2
    return lo, hi


def validate(nodes, leaf_parent, nleaf, leaf_boxes=None, nodes4=None):
    """Every violation of a built hierarchy as a list of strings (empty: valid).  `nodes` is a NODE
    array, `leaf_boxes` [nleaf, 6] the leaf clusters' boxes, `nodes4` a NODE4 array."""
    out = []
    nn = nodes.shape[0]
    child = nodes["child"].astype(np.int64)
    parent = nodes["parent"].astype(np.int64)
    leaf_parent = np.asarray(leaf_parent, np.int64)
    if nn != max(nleaf - 1, 1):
        return [f"{nn} nodes for {nleaf} leaves"]
    if nleaf == 1:
        if tuple(child[0]) != (~0, EMPTY_CHILD) or parent[0] != -1 or nodes["nleaf"][0] != 1:
            out.append("single leaf: not the (~0, empty) root")
        if leaf_boxes is not None:
            lb = np.ascontiguousarray(leaf_boxes, np.float32).reshape(1, 6)
            want_lo = np.stack([lb[0, :3], np.full(3, FLT_MAX, np.float32)])
            want_hi = np.stack([lb[0, 3:], np.full(3, -FLT_MAX, np.float32)])
            if not (np.array_equal(_bits(nodes["lo"][0]), _bits(want_lo))
                    and np.array_equal(_bits(nodes["hi"][0]), _bits(want_hi))):
                out.append("single leaf: boxes")
        if nodes4 is not None and nodes4.tobytes() != collapse4(nodes).tobytes():
            out.append("nodes4 differs from collapse4")
        return out
    # 1. every leaf and every interior node once from node 0: preorder, left child first
    seen_node = np.zeros(nn, np.int64)
    seen_leaf = np.zeros(nleaf, np.int64)
    order, leaf_order = [], []
    depth_of = np.zeros(nn, np.int64)
    stack = [(0, 0)]
    steps, max_depth = 0, 0
    while stack and steps < 2 * nleaf:
        c, dep = stack.pop()
        steps += 1
        if c == EMPTY_CHILD:
            out.append("an empty child in a tree of several leaves")
        elif c < 0:
            if ~c >= nleaf:
                out.append(f"leaf {~c} out of range")
            else:
                seen_leaf[~c] += 1
                leaf_order.append(~c)
        elif c >= nn:
            out.append(f"node {c} out of range")
        else:
            seen_node[c] += 1
            if seen_node[c] == 1:
                order.append(c)
                depth_of[c] = dep
                max_depth = max(max_depth, dep)
                stack.append((int(child[c, 1]), dep + 1))
                stack.append((int(child[c, 0]), dep + 1))
    if stack:
        out.append(f"the walk from the root did not end in {2 * nleaf} steps")
    bad = np.nonzero(seen_leaf != 1)[0]
    if bad.size:
        out.append(f"{bad.size} leaves not reached exactly once (first {bad[0]}: {seen_leaf[bad[0]]} times)")
    bad = np.nonzero(seen_node != 1)[0]
    if bad.size:
        out.append(f"{bad.size} nodes not reached exactly once (first {bad[0]}: {seen_node[bad[0]]} times)")
    if max_depth + 1 > MAX_DEPTH:
        out.append(f"depth {max_depth + 1} > {MAX_DEPTH} (traversal stack {STACK_DEPTH})")
    # 2. parent and leaf_parent agree with child
    if parent[0] != -1:
        out.append(f"root parent {parent[0]}")
    for s in (0, 1):
        c = child[:, s]
        it = (c >= 0) & (c < nn)
        wrong = np.nonzero(parent[c[it]] != np.nonzero(it)[0])[0]
        if wrong.size:
            out.append(f"{wrong.size} parent words disagree with child[{s}] (first: node {c[it][wrong[0]]})")
        lf = (c < 0) & (c != EMPTY_CHILD) & (~c < nleaf)
        wrong = np.nonzero(leaf_parent[~c[lf]] != np.nonzero(lf)[0])[0]
        if wrong.size:
            out.append(f"{wrong.size} leaf_parent words disagree with child[{s}] (first: leaf {~c[lf][wrong[0]]})")
    # 3. every leaf-to-root walk ends at -1 within nleaf steps
    p = leaf_parent.copy()
    for _ in range(nleaf):
        live = p >= 0
        if not live.any():
            break
        over = live & (p >= nn)
        p[over] = -3
        live &= ~over
        p[live] = parent[p[live]]
    bad = np.nonzero(p != -1)[0]
    if bad.size:
        out.append(f"{bad.size} leaf-to-root walks do not end at the root (first: leaf {bad[0]})")
    if out:
        return out  # the range and box checks below need a tree
    # 4. contiguous ranges, left before right, nleaf_below
    first = np.zeros(nn, np.int64)
    last = np.zeros(nn, np.int64)
    for c in reversed(order):
        rng = []
        for s in (0, 1):
            ch = int(child[c, s])
            rng.append((~ch, ~ch) if ch < 0 else (int(first[ch]), int(last[ch])))
        if rng[0][1] + 1 != rng[1][0]:
            out.append(f"node {c}: child ranges {rng[0]} and {rng[1]} are not adjacent, left first")
        first[c], last[c] = rng[0][0], rng[1][1]
        if last[c] - first[c] + 1 != nodes["nleaf"][c]:
            out.append(f"node {c}: nleaf {nodes['nleaf'][c]} but leaves [{first[c]}, {last[c]}]")
    if leaf_order != list(range(nleaf)):
        out.append("the left-to-right walk does not visit the leaves in order")
    if out:
        return out
    # 5. each child box is the exact union of the leaf boxes below it (range queries on the leaves,
    # not the bottom-up carry of refit)
    if leaf_boxes is not None:
        lb = np.ascontiguousarray(leaf_boxes, np.float32).reshape(nleaf, 6)
        tlo, thi = _range_min_tables(lb)
        for s in (0, 1):
            c = child[:, s]
            a = np.where(c < 0, ~c, first[np.maximum(c, 0)])
            b = np.where(c < 0, ~c, last[np.maximum(c, 0)])
            k = _bit_length(b - a + 1) - 1
            want_lo = np.empty((nn, 3), np.float32)
            want_hi = np.empty((nn, 3), np.float32)
            for lev in np.unique(k):
                m = k == lev
                w = 1 << int(lev)
                want_lo[m] = np.minimum(tlo[lev][a[m]], tlo[lev][b[m] - w + 1])
                want_hi[m] = np.maximum(thi[lev][a[m]], thi[lev][b[m] - w + 1])
            bad = np.nonzero((_bits(want_lo) != _bits(nodes["lo"][:, s])).any(axis=1)
                             | (_bits(want_hi) != _bits(nodes["hi"][:, s])).any(axis=1))[0]
            if bad.size:
                out.append(f"{bad.size} child-{s} boxes are not the union of their leaves (first: node {bad[0]})")
    # 6. the 4-wide view
    if nodes4 is not None:
        want = collapse4(nodes)
        if nodes4.shape != want.shape:
            out.append(f"nodes4 has {nodes4.shape[0]} records for {nn} nodes")
        else:
            bad = [i for i in range(nn) if nodes4[i].tobytes() != want[i].tobytes()]
            if bad:
                out.append(f"{len(bad)} Node4 records differ from collapse4 (first: node {bad[0]})")
    return out
