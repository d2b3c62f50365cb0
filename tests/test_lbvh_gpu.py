"""The beam BVH the GPU builds (bre_build.hip k_karras / k_refit / k_single, bre_roots.hip k_collapse4)
against the host restatement and validator of tests/refpy_lbvh.py, word for word.

* bre_device_check kind 10 runs the hierarchy kernels on the key sets of tests/test_lbvh_host.py (every
  valid one: ties, single bits, ragged leaves, keys sorted on bits [16, 64) only and compared from bit 16)
  and random boxes.
* kind 11 reads real builds back (tree keys 0 / 1 / 2, tile leaves 1 / 7 / 64, kernel 2 leaves 1 / 4) over
  random, duplicate, lattice, planar and partly invalid beam sets: the sort order, the index permutation,
  the equal-centroid group boxes against oracle.beam_bounds, the topology, the boxes, the 4-wide view.
* The two tie-heaviest sets gathered end to end against the brute force.
* One build with coarse sort keys on (internal option 121).

Everything is compared exactly: integers, and boxes bit for bit (min and max do not round)."""
import ctypes

import numpy as np
import pytest

import refpy_lbvh as L
from test_lbvh_host import COARSE, KEY_SETS, coarse_keys, random_boxes

pytestmark = pytest.mark.gpu


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def compare_tree(nodes, leaf_parent, nodes4, keys, boxes, leaf_size, key_lo):
    """The GPU's records against karras / refit / collapse4 of the same keys and member boxes."""
    topo = L.karras(keys, leaf_size, key_lo)
    assert topo["problems"] == []
    nleaf = topo["leaf_parent"].shape[0]
    lb = L.leaf_boxes(boxes, leaf_size)
    assert nodes.shape[0] == topo["child"].shape[0]
    assert np.array_equal(nodes["child"], topo["child"])
    assert np.array_equal(nodes["parent"], topo["parent"])
    assert np.array_equal(nodes["nleaf"], topo["nleaf_below"])
    assert np.array_equal(leaf_parent, topo["leaf_parent"])
    lo, hi = L.refit(topo["child"], lb)
    assert same_bits(nodes["lo"], lo) and same_bits(nodes["hi"], hi)
    # validate() holds nodes4 against collapse4(nodes) record by record
    assert L.validate(nodes, leaf_parent, nleaf, lb, nodes4) == []
    return nleaf


# ---- kind 10: the hierarchy kernels on caller data ----
@pytest.fixture(scope="module")
def ctx(bre):
    with bre.BeamGather(0) as g:
        yield g


@pytest.mark.parametrize("name", list(KEY_SETS))
def test_hierarchy_kernels_match_restatement(ctx, name):
    keys, leaf_size, key_lo = KEY_SETS[name]
    assert keys.shape[0] <= 8192
    boxes = random_boxes(keys.shape[0], 1000 + keys.shape[0])
    got = ctx.hierarchy_check(keys, boxes, leaf_size, key_lo)
    nleaf = compare_tree(got["nodes"], got["leaf_parent"], got["nodes4"], keys, boxes, leaf_size, key_lo)
    assert nleaf == (keys.shape[0] + leaf_size - 1) // leaf_size


def test_non_monotone_keys_are_refused_before_any_launch(bre):
    n, d, seed = COARSE[1]
    keys = coarse_keys(n, d, seed)  # ordered from bit 16 up only
    boxes = random_boxes(n, 3)
    with bre.BeamGather(0) as g:
        with pytest.raises(bre.BreError) as e:
            g.hierarchy_check(keys, boxes, 1, 0)
        assert e.value.status == 1  # BRE_ERR_INVALID_ARG
        # the context is still usable: the same keys from the bit they are ordered from, then a gather
        got = g.hierarchy_check(keys, boxes, 1, 16)
        compare_tree(got["nodes"], got["leaf_parent"], got["nodes4"], keys, boxes, 1, 16)
        g.set_beams(np.array([[0, 0, 0]], np.float32), np.array([[1, 1, 1]], np.float32),
                    np.array([0.01], np.float32), np.ones((1, 3), np.float32))
        assert g.read_tree()["nvalid"] == 1


# ---- kind 11: real builds ----
def _lattice(n, seed):
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 8, size=n)
    b = (a + rng.integers(1, 8, size=n)) % 8  # another corner: no zero-length beam
    corner = lambda c: np.stack([c & 1, (c >> 1) & 1, (c >> 2) & 1], axis=1).astype(np.float32)  # noqa: E731
    return {"start": corner(a), "end": corner(b),
            "radius": np.where(np.arange(n) % 2 == 0, 0.01, 0.02).astype(np.float32),  # groups of unequal boxes
            "power": rng.random((n, 3), dtype=np.float32)}


def _beam_set(synth, name):
    if name.startswith("fog-"):
        return synth.fog_beams(int(name[4:]), seed=4242)
    if name == "copies-4097":
        one = {"start": [[0.1, 0.2, 0.3]], "end": [[0.9, 0.7, 0.6]], "radius": [0.02], "power": [[0.5, 0.25, 1.0]]}
        return {k: np.repeat(np.asarray(v, np.float32), 4097, axis=0) for k, v in one.items()}
    if name == "lattice-3000":
        return _lattice(3000, 5)
    if name == "plane-1500":
        b = synth.fog_beams(1500, seed=6)
        b["start"][:, 2] = 0.5
        b["end"][:, 2] = 0.5
        return b
    if name == "third-invalid-999":
        b = synth.fog_beams(999, seed=7)
        b["end"][::3] = b["start"][::3]  # zero length: WorldBound is NaN, the beam is left out
        return b
    raise KeyError(name)


BEAM_SETS = ["fog-1", "fog-2", "fog-64", "fog-65", "fog-5000", "copies-4097", "lattice-3000", "plane-1500",
             "third-invalid-999"]
_CACHE = {}


def case_of(oracle, b):
    """A beam set with its valid input indices and every beam's equal-centroid group box."""
    with np.errstate(invalid="ignore"):
        box = oracle.beam_bounds(b["start"], b["end"], b["radius"])
        cent = np.float32(0.5) * box[:, :3] + np.float32(0.5) * box[:, 3:]
    valid = np.isfinite(box).all(axis=1) & np.isfinite(cent).all(axis=1)
    gbox = box.copy()
    vi = np.nonzero(valid)[0]
    _, inv = np.unique(cent[vi] + np.float32(0), axis=0, return_inverse=True)  # -0 == +0
    inv = inv.ravel()
    glo = np.full((inv.max() + 1, 3), np.inf, np.float32)
    ghi = np.full((inv.max() + 1, 3), -np.inf, np.float32)
    np.minimum.at(glo, inv, box[vi, :3])
    np.maximum.at(ghi, inv, box[vi, 3:])
    gbox[vi, :3], gbox[vi, 3:] = glo[inv], ghi[inv]
    grown = bool((gbox[vi] != box[vi]).any())  # some group's box is larger than a member's own
    return (b, vi, gbox, int(inv.max() + 1), grown)


def beam_case(synth, oracle, name):
    """The named set's case_of, computed once."""
    if name not in _CACHE:
        _CACHE[name] = case_of(oracle, _beam_set(synth, name))
    return _CACHE[name]


# (kernel, tree key (internal option 110), BRE_OPT_TILE_LEAF, BRE_OPT_LEAF_SIZE)
CONFIGS = {"k0-key0-tile1": (0, 0, 1, None), "k0-key1-tile1": (0, 1, 1, None), "k0-key2-tile1": (0, 2, 1, None),
           "k0-key2-tile7": (0, 2, 7, None), "k0-key2-tile64": (0, 2, 64, None),
           "k2-leaf1": (2, 2, None, 1), "k2-leaf4": (2, 2, None, 4)}


def _configure(bre, g, cfg):
    kernel, tree_key, tile_leaf, leaf = CONFIGS[cfg]
    g.set_option(bre.OPT_KERNEL, kernel)
    g.set_option(110, tree_key)
    if tile_leaf is not None:
        g.set_option(bre.OPT_TILE_LEAF, tile_leaf)
    if leaf is not None:
        g.set_option(bre.OPT_LEAF_SIZE, leaf)
    return tile_leaf if kernel == 0 else leaf


def check_build(g, case, leaf_size, key_lo, has4):
    b = case[0]
    g.set_beams(b["start"], b["end"], b["radius"], b["power"])
    return check_tree(g, case, leaf_size, key_lo, has4)


def check_tree(g, case, leaf_size, key_lo, has4):
    """The context's current build (of case's beams, however they were set) against the restatement."""
    b, vi, gbox = case[:3]
    t = g.read_tree()
    st = g.stats()
    nv = vi.shape[0]
    assert t["nvalid"] == nv == st["n_beams_valid"] and st["n_beams"] == b["radius"].shape[0]
    assert t["leaf_size"] == leaf_size and t["key_lo"] == key_lo
    top = t["keys"] >> np.uint64(key_lo)
    assert (top[1:] >= top[:-1]).all(), "keys >> key_lo decrease"
    assert np.array_equal(np.sort(t["index"]), vi), "not a permutation of the valid beams"
    assert same_bits(t["boxes"], gbox[t["index"]]), "a record's box is not its equal-centroid group's"
    assert (t["nodes4"] is not None) == has4
    nleaf = compare_tree(t["nodes"], t["leaf_parent"], t["nodes4"], t["keys"], t["boxes"], leaf_size, key_lo)
    assert t["nleaf"] == nleaf == (nv + leaf_size - 1) // leaf_size
    assert st["n_nodes"] == max(nleaf - 1, 1) == t["nodes"].shape[0]
    return t


@pytest.mark.parametrize("beams", BEAM_SETS)
@pytest.mark.parametrize("cfg", list(CONFIGS))
def test_built_tree_matches_restatement(bre, synth, oracle, cfg, beams):
    case = beam_case(synth, oracle, beams)
    assert case[0]["radius"].shape[0] <= 20000
    with bre.BeamGather(0) as g:
        leaf_size = _configure(bre, g, cfg)
        check_build(g, case, leaf_size, 0, has4=CONFIGS[cfg][0] == 0)


def test_tie_heavy_sets_have_few_keys(bre, synth, oracle):
    """What the two tie-heaviest sets are there for: one key for the copies, a handful for the lattice
    (under every tree key), and more than one equal-centroid group with unequal member boxes."""
    for name, most in (("copies-4097", 1), ("lattice-3000", 56)):
        case = beam_case(synth, oracle, name)
        for tree_key in (0, 1, 2):
            with bre.BeamGather(0) as g:
                g.set_option(110, tree_key)
                g.set_option(bre.OPT_TILE_LEAF, 1)
                g.set_beams(*(case[0][k] for k in ("start", "end", "radius", "power")))
                keys = g.read_tree()["keys"]
            assert np.unique(keys).shape[0] <= most, (name, tree_key)
    lat = beam_case(synth, oracle, "lattice-3000")
    assert lat[3] <= 56 and lat[4]


def test_read_tree_refuses_a_short_buffer(bre, synth):
    b = synth.fog_beams(100, seed=1)
    with bre.BeamGather(0) as g:
        g.set_beams(b["start"], b["end"], b["radius"], b["power"])
        y = np.zeros(64, np.uint32)
        st = g.lib.bre_device_check(g.h, 11, y.shape[0], None, 0, None, ctypes.c_void_p(y.ctypes.data))
        assert st == 1 and not y.any()  # BRE_ERR_INVALID_ARG, nothing written
        assert g.read_tree()["nvalid"] == 100


# ---- end to end on the tie-heaviest sets ----
@pytest.mark.parametrize("kernel", [0, 2])
@pytest.mark.parametrize("beams", ["copies-4097", "lattice-3000"])
def test_tie_heavy_sets_gather_like_the_brute_force(bre, synth, oracle, beams, kernel):
    b = beam_case(synth, oracle, beams)[0]
    segs = synth.bounce_segments(2000, seed=31)
    R = 0.02
    key = ("bf", beams)
    if key not in _CACHE:
        _CACHE[key] = oracle.bruteforce(b, segs, R, nthreads=8)
    bf = _CACHE[key]
    assert bf["cand"].sum() > 0 and bf["contrib"].sum() > 0
    with bre.BeamGather(0, counters=True, kernel=kernel, leaf_size=1) as g:
        g.set_option(bre.OPT_TILE_LEAF, 1)
        g.set_beams(b["start"], b["end"], b["radius"], b["power"])
        out = g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], R=R, counts=True)
    assert np.array_equal(out["counts"][:, 0], bf["cand"]), "candidate counts differ"
    assert np.array_equal(out["counts"][:, 1], bf["contrib"]), "contribution counts differ"


# ---- coarse sort keys (internal option 121) ----
def test_coarse_keys_build(bre, synth, oracle):
    """The tree-order sort on bits [16, 64) only and the hierarchy comparing from bit 16 (the fixed form
    of round 6's coarse keys; tests/test_lbvh_host.py shows on the host that this form gives a valid tree
    and the first form did not).  The same checks as every other build, with key_lo == 16; whether the
    low 16 bits happened to come out sorted is printed, not asserted (on an MI355X they did for both sets:
    the lattice's keys have equal low bits, and no two of the 5000 random beams tie in the top 48 bits;
    ties with unsorted low bits reach the kernels through kind 10's coarse key sets above)."""
    for name in ("lattice-3000", "fog-5000"):
        case = beam_case(synth, oracle, name)
        with bre.BeamGather(0) as g:
            g.set_option(121, 1)
            g.set_option(bre.OPT_TILE_LEAF, 1)
            t = check_build(g, case, 1, 16, has4=True)
        k = t["keys"]
        print(f"coarse keys, {name}: low 16 bits sorted within the top-bit runs: {bool((k[1:] >= k[:-1]).all())}")
