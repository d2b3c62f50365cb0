"""The LBVH hierarchy on the host: the restatement of k_karras / k_refit / k_collapse4 and the tree
validator of tests/refpy_lbvh.py.

1. The cause of round 6's coarse-keys hang, shown without a GPU: keys sorted
   on bits [16, 64) only give a valid tree when the split compares `keys >> 16` (the fixed form) and
   an invalid one when it compares all 64 bits (the first form): RECORDED holds what goes wrong at
   each size.
2. Edge shapes of the key sequence, all of which must give a valid tree.
3. The validator reports every single mutation of a valid tree.

KEY_SETS is shared with tests/test_lbvh_gpu.py, which runs the same sets through the kernels.
"""
import numpy as np
import pytest

import refpy_lbvh as L

COARSE = [(64, 4, 11), (1000, 10, 12), (5000, 3, 13), (5000, 2000, 14)]  # (n, distinct top values, seed)
RECORDED = {}  # (n, d) -> the violations of the pre-fix comparison (printed with -s / on failure)


def coarse_keys(n, d, seed):
    """n keys with d distinct values in bits [16, 64) and random low 16 bits, sorted (stably) on the top
    48 bits only: what the hierarchy reads behind a coarse tree-order sort."""
    rng = np.random.default_rng(seed)
    tops = np.unique(rng.integers(0, 1 << 44, size=4 * d + 8, dtype=np.uint64))
    tops = rng.permutation(tops)[:d]
    assert tops.shape[0] == d
    keys = (tops[rng.integers(0, d, size=n)] << np.uint64(16)) | rng.integers(0, 1 << 16, size=n, dtype=np.uint64)
    keys = keys[np.argsort(keys >> np.uint64(16), kind="stable")]
    assert (np.diff((keys >> np.uint64(16)).astype(np.int64)) >= 0).all()
    assert (keys[1:] < keys[:-1]).any(), "the low bits came out sorted: not the case under test"
    return keys


def random_boxes(m, seed):
    rng = np.random.default_rng(seed)
    lo = rng.random((m, 3), dtype=np.float32)
    ext = rng.random((m, 3), dtype=np.float32) * np.float32(0.1)
    return np.concatenate([lo, lo + ext], axis=1).astype(np.float32)


def bare_nodes(topo):
    nodes = np.zeros(topo["child"].shape[0], L.NODE)
    nodes["child"], nodes["parent"], nodes["nleaf"] = topo["child"], topo["parent"], topo["nleaf_below"]
    return nodes


def violations(keys, leaf_size, key_lo):
    """karras()'s out-of-range writes plus validate() of the topology it leaves."""
    topo = L.karras(keys, leaf_size, key_lo)
    nleaf = topo["leaf_parent"].shape[0]
    return topo["problems"] + L.validate(bare_nodes(topo), topo["leaf_parent"], nleaf)


def full_check(keys, leaf_size, key_lo, seed=5):
    """A valid key sequence: clean topology, and clean boxes / 4-wide view over random member boxes."""
    keys = np.asarray(keys, np.uint64)
    assert violations(keys, leaf_size, key_lo) == []
    boxes = random_boxes(keys.shape[0], seed)
    nodes, leaf_parent, nodes4 = L.build(keys, boxes, leaf_size, key_lo)
    nleaf = leaf_parent.shape[0]
    assert nleaf == (keys.shape[0] + leaf_size - 1) // leaf_size
    assert L.validate(nodes, leaf_parent, nleaf, L.leaf_boxes(boxes, leaf_size), nodes4) == []
    if nleaf > 1:
        # the root's two boxes together are the box of everything
        assert np.array_equal(nodes["lo"][0].min(axis=0), boxes[:, :3].min(axis=0))
        assert np.array_equal(nodes["hi"][0].max(axis=0), boxes[:, 3:].max(axis=0))


# ---- the key sets (name -> (keys, leaf_size, key_lo)), every one a valid input of the hierarchy ----
def _distinct(n, seed):
    rng = np.random.default_rng(seed)
    k = np.unique(rng.integers(0, 1 << 60, size=2 * n + 8, dtype=np.uint64))
    return np.sort(rng.permutation(k)[:n])


def _one_bit(n, bit):
    base = np.uint64(0x0123456789ABCDE0) & ~(np.uint64(1) << np.uint64(bit))
    k = np.full(n, base, np.uint64)
    k[n // 3:] |= np.uint64(1) << np.uint64(bit)
    return k


def _tie_runs():
    runs = []
    for k in range(1, 7):
        runs += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    vals = _distinct(len(runs), 21)
    return np.repeat(vals, runs)


def _ties(n, d, seed):
    rng = np.random.default_rng(seed)
    return np.sort(_distinct(d, seed)[rng.integers(0, d, size=n)])


def key_sets():
    sets = {}
    for (n, d, seed) in COARSE:
        k = coarse_keys(n, d, seed)
        sets[f"coarse-{n}-{d}-lo16"] = (k, 1, 16)
        sets[f"coarse-{n}-{d}-sorted"] = (np.sort(k), 1, 0)
    for nleaf in (1, 2, 3, 64, 65, 4097):
        sets[f"distinct-{nleaf}"] = (_distinct(nleaf, 30 + nleaf), 1, 0)
    sets["all-equal-100"] = (np.full(100, 0x0FEDCBA987654321, np.uint64), 1, 0)
    sets["all-equal-4097"] = (np.full(4097, 7, np.uint64), 1, 0)
    for bit in (0, 59, 62):
        sets[f"bit{bit}-only"] = (_one_bit(257, bit), 1, 0)
    sets["tie-runs"] = (_tie_runs(), 1, 0)
    for ls in (1, 3, 64):
        sets[f"ragged-leaf{ls}"] = (_ties(1000, 37, 40 + ls), ls, 0)  # 1000 = 333 * 3 + 1 = 15 * 64 + 40
    sets["ragged-leaf3-one-short"] = (_ties(1001, 500, 44), 3, 0)
    sets["leaf64-single"] = (_ties(40, 9, 45), 64, 0)
    sets["coarse-ragged-leaf3"] = (coarse_keys(1000, 10, 12), 3, 16)
    return sets


KEY_SETS = key_sets()


@pytest.mark.parametrize("n,d,seed", COARSE)
def test_coarse_keys_fixed_form_is_valid_first_form_is_not(n, d, seed):
    keys = coarse_keys(n, d, seed)
    # the fixed form: the comparison sees the bits the sort ordered
    full_check(keys, 1, 16)
    # fully sorted keys, all bits compared
    full_check(np.sort(keys), 1, 0)
    # the first form: all 64 bits compared although only [16, 64) are ordered
    topo = L.karras(keys, 1, 0)
    v = violations(keys, 1, 0)
    RECORDED[(n, d)] = v
    print(f"coarse keys n={n} d={d}, all bits compared: {len(v)} violations")
    for line in v[:12]:
        print("   ", line)
    assert len(v) >= 1
    # what round 6's diagnosis names: the leaves are not each reached once, the parent walks do not all
    # end at the root
    assert any("leaves not reached exactly once" in s for s in v)
    assert any("leaf-to-root walks do not end at the root" in s for s in v)
    # and every loop of the restatement ended (the kernel's build loops are bounded by the index width;
    # the loops without a bound are k_refit's and the tile walk's, which read this tree)
    assert not any("did not end" in s for s in topo["problems"])


def test_first_form_writes_one_record_past_the_node_array():
    """When the last three leaves' unsorted low bits go high, low, high, the last node i = nleaf - 2
    shares the same prefix with both neighbours: its range search finds length 0 (j == i), the right
    child becomes *interior* node i + 1 = nleaf - 1, and k_karras writes nodes[nleaf - 1].parent, one
    record past its nleaf - 1 nodes.  By hand on three keys, then in the random sets whose tail has
    that pattern (1000 / 10 and 5000 / 3; the other two seeds end differently)."""
    top = np.uint64(0xABCDEF) << np.uint64(16)
    keys = top | np.array([1, 0, 1], np.uint64)  # sorted on bits [16, 64)
    t = L.karras(keys, 1, 0)
    assert t["problems"] == ["node 1: child 1 is interior node 2: nodes[2].parent written one record past the "
                             "node array (2 nodes)"]
    assert t["child"].tolist()[1] == [~1, 2]
    assert L.karras(keys, 1, 16)["problems"] == []
    for (n, d, seed) in ((1000, 10, 12), (5000, 3, 13)):
        keys = coarse_keys(n, d, seed)
        past = [s for s in L.karras(keys, 1, 0)["problems"] if "one record past the node array" in s]
        assert past == [f"node {n - 2}: child 1 is interior node {n - 1}: nodes[{n - 1}].parent written one record "
                        f"past the node array ({n - 1} nodes)"]
        assert L.karras(keys, 1, 16)["problems"] == []


@pytest.mark.parametrize("name", [k for k in KEY_SETS if not k.startswith("coarse-")])
def test_edge_shapes_are_valid(name):
    keys, leaf_size, key_lo = KEY_SETS[name]
    full_check(keys, leaf_size, key_lo)


def test_coarse_ragged_leaf_is_valid():
    full_check(*KEY_SETS["coarse-ragged-leaf3"])


def test_single_leaf_conventions():
    t = L.karras(np.array([5, 5, 9], np.uint64), leaf_size=64)
    assert t["child"].tolist() == [[~0, L.EMPTY_CHILD]] and t["parent"].tolist() == [-1]
    assert t["nleaf_below"].tolist() == [1]
    boxes = random_boxes(3, 1)
    nodes, leaf_parent, nodes4 = L.build(np.array([5, 5, 9], np.uint64), boxes, 64)
    assert np.array_equal(nodes["lo"][0, 0], boxes[:, :3].min(axis=0))
    assert np.array_equal(nodes["hi"][0, 1], np.full(3, -L.FLT_MAX, np.float32))
    assert nodes4["child"][0].tolist() == [~0] + [L.EMPTY_CHILD] * 3
    assert not nodes4["lo"][0][:, 1:].any() and not nodes4["pad"].any()


def test_two_and_three_leaves_by_hand():
    t = L.karras(np.array([1, 2], np.uint64))
    assert t["child"].tolist() == [[~0, ~1]] and t["leaf_parent"].tolist() == [0, 0]
    # 0b001, 0b010, 0b011: the top split is after leaf 0, node 1 holds leaves 1 and 2
    t = L.karras(np.array([1, 2, 3], np.uint64))
    assert t["child"].tolist() == [[~0, 1], [~1, ~2]]
    assert t["parent"].tolist() == [-1, 0] and t["nleaf_below"].tolist() == [3, 2]
    assert t["leaf_parent"].tolist() == [0, 1, 1]
    # equal keys split by index: clz32(i ^ j) of 0..3 splits 0,1 | 2,3
    t = L.karras(np.full(4, 9, np.uint64))
    assert t["child"].tolist() == [[1, 2], [~0, ~1], [~2, ~3]]


def test_equal_keys_tree_is_shallow():
    """The index tie-break makes a run of equal keys a balanced subtree, not a chain: 4097 equal keys
    stay far inside the traversal stack."""
    nodes, leaf_parent, _ = L.build(np.full(4097, 7, np.uint64), random_boxes(4097, 2))
    assert L.validate(nodes, leaf_parent, 4097) == []
    p, depth = leaf_parent.astype(np.int64), 0
    while (p >= 0).any() and depth < 200:
        p = np.where(p >= 0, nodes["parent"][np.maximum(p, 0)], p)
        depth += 1
    assert depth <= 14


# ---- the validator has teeth ----
@pytest.fixture(scope="module")
def valid_tree():
    keys = _ties(300, 40, 77)
    boxes = random_boxes(300, 78)
    nodes, leaf_parent, nodes4 = L.build(keys, boxes, 1, 0)
    lb = L.leaf_boxes(boxes, 1)
    assert L.validate(nodes, leaf_parent, 300, lb, nodes4) == []
    return nodes, leaf_parent, nodes4, lb


def _interior_with(nodes, want):
    for i in range(nodes.shape[0]):
        if want(nodes[i]):
            return i
    raise AssertionError("no such node in the fixture tree")


def _mutants(nodes, leaf_parent, nodes4):
    """(name, nodes, leaf_parent, nodes4) with exactly one thing wrong each."""
    n = nodes.copy()
    i = _interior_with(n, lambda r: r["child"][0] >= 0 and r["child"][1] >= 0)
    n["child"][i] = n["child"][i][::-1].copy()
    n["lo"][i] = n["lo"][i][::-1].copy()  # boxes follow their child: only the order is wrong
    n["hi"][i] = n["hi"][i][::-1].copy()
    yield "children swapped", n, leaf_parent, L.collapse4(n)
    for dlt in (1, -1):
        n = nodes.copy()
        n["nleaf"][nodes.shape[0] // 2] += dlt
        yield f"nleaf_below off by {dlt}", n, leaf_parent, nodes4
    n = nodes.copy()
    i = _interior_with(n, lambda r: r["parent"] > 0)
    n["parent"][i] = 0 if n["parent"][i] != 0 else 1
    yield "parent redirected", n, leaf_parent, nodes4
    lp = leaf_parent.copy()
    lp[17] = lp[200]
    yield "leaf_parent redirected", nodes, lp, nodes4
    n = nodes.copy()
    i = _interior_with(n, lambda r: r["child"][0] < 0 and r["child"][1] < 0 and r["child"][0] != ~0)
    n["child"][i][1] = ~0  # leaf 0 now hangs here too, this node's own second leaf is lost
    yield "leaf referenced twice", n, leaf_parent, L.collapse4(n)
    for field, towards in (("lo", np.inf), ("hi", -np.inf)):
        n = nodes.copy()
        i, s, a = nodes.shape[0] // 3, 1, 2
        n[field][i, s, a] = np.nextafter(n[field][i, s, a], np.float32(towards))
        yield f"{field} one ulp inwards", n, leaf_parent, L.collapse4(n)
    q = nodes4.copy()
    i = _interior_with(nodes, lambda r: r["child"][0] >= 0 and r["child"][1] >= 0)
    for f in ("lo", "hi"):
        q[f][i][:, [1, 2]] = q[f][i][:, [2, 1]]
    q["child"][i][[1, 2]] = q["child"][i][[2, 1]]
    yield "Node4 slots permuted", nodes, leaf_parent, q
    q = nodes4.copy()
    q["pad"][5][0] = 1
    yield "Node4 pad word set", nodes, leaf_parent, q


def test_validator_reports_every_mutation(valid_tree):
    nodes, leaf_parent, nodes4, lb = valid_tree
    names = []
    for name, n, lp, q in _mutants(nodes, leaf_parent, nodes4):
        v = L.validate(n, lp, 300, lb, q)
        assert v, f"mutation not reported: {name}"
        names.append(name)
    assert len(names) == 10
    assert L.validate(nodes, leaf_parent, 300, lb, nodes4) == []  # the fixture itself was not touched


def test_validator_bounds_its_walks_on_a_cycle(valid_tree):
    """A node made its own ancestor: the walks stop at their caps and say so."""
    nodes, leaf_parent, nodes4, lb = valid_tree
    n = nodes.copy()
    i = _interior_with(n, lambda r: r["child"][0] >= 0 and r["parent"] > 0)
    n["child"][i][0] = 0
    v = L.validate(n, leaf_parent, 300, lb, None)
    assert any("not reached exactly once" in s for s in v)
    n = nodes.copy()
    n["parent"][i] = i
    v = L.validate(n, leaf_parent, 300, lb, None)
    assert any("do not end at the root" in s for s in v)
