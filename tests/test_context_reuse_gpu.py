"""One long-lived context (bre_ctx) through resizes, option changes and mixed entry points.

A caller holds one context for a whole render (the pbrt adapter, bench.py's SceneWorkload); the context keeps
~90 device buffers that only grow and caches derived state behind flags and keys (roots_split, nodes4_ok,
build_scratch_ok, beams_kept, built_leaf_size, built_key_lo, bset.uniform, cam_w / cam_h / cam_scene, sc_hash +
sc_bytes, ph_scene_host, grid_bytes, the sticky DevCounters::flags word, counters_buf).  Every other GPU test
opens a fresh context per build; these walks keep one context `g` alive and, after each step, repeat that step
alone on a fresh context `f` with g's options of that moment.  Nothing in a result may depend on a buffer's
capacity or on what ran before, so g and f must agree BIT FOR BIT (per-segment sums and counts for every
kernel, films for kernels 0 and 4 whose compose is deterministic; kernels 2 and 5 add to the film by float
atomics and their films are not compared), and in n_beams / n_beams_valid / n_nodes / n_segments (candidates /
contributions with counters on).  Every step with counters on is also held against the CPU oracle at the bar of
tests/test_gpu_parity.py (exact counts, SEG_RTOL), so the walks are not only self-referential, and every step
that has a valid beam and a segment must contribute in the oracle alone (ctx_walk.oracle_ref asserts it).

Kernel 5 enumerates capsule chunks, not the reference's candidates (tests/test_radius_layout_gpu.py): its
counts[:, 0] is not held against the oracle's C; its contributions and sums are.  Its per-segment sums turned
out independent of what ran before (bit-equal to a fresh context's), so it stays on the bit-for-bit bar.

Walks: A the beam set grows, shrinks, empties and changes layout; B the segment set changes on one build;
C BRE_OPT_KERNEL changes between the build and the gather; D options change on a live context; E the scene,
medium and film caches of the photon and camera passes; F refused calls leave the context as it was."""
import numpy as np
import pytest

import ctx_walk as W
from test_camera_gpu import _assert_segments_equal
from test_lbvh_gpu import case_of, check_tree
from test_photon_gpu import _assert_beams_equal

pytestmark = pytest.mark.gpu

NPIX = 1024
_REF = {}  # oracle results, computed once and shared by the walks


def _cached(key, make):
    if key not in _REF:
        _REF[key] = make()
    return _REF[key]


def _segs(synth, n, seed=None):
    if n == 0:
        return W.empty_segments()
    return _cached(("segs", n, seed), lambda: synth.bounce_segments(n, seed=n if seed is None else seed, npix=NPIX))


def _beams(synth, name):
    return _cached(("beams", name), lambda: W.beams_of(synth, name))


def _ref(synth, oracle, name, segs_key, R, sqrt_mode=0):
    """The oracle's gather of a named beam set and a segment set ((n, seed) of _segs)."""
    return _cached(("ref", name, segs_key, R, sqrt_mode),
                   lambda: W.oracle_ref(oracle, _beams(synth, name), _segs(synth, *segs_key), R, sqrt_mode))


# ---- walk A ----
A_STEPS = [("fog-5000", 0.01), ("fog-17", 0.05), ("empty", 0.05), ("fog-1", 0.05), ("fog-20000", 0.01),
           ("fog-64", 0.05), ("fog-65", 0.05), ("third-invalid-999", 0.01), ("degenerate-50", 0.05),
           ("fog-3000-radii", 0.013), ("fog-3000", 0.013), ("fog-5000", 0.01)]
A_TREE = (0, 4, 5, 9)  # the steps whose tree is read back and held against the host restatement
# the oracle's candidate / contribution totals of the steps' inputs (computed on the CPU): pins the inputs
A_TOTALS = {"fog-5000": (147392, 35957), "fog-17": (1964, 646), "fog-1": (7, 7), "fog-20000": (587516, 143288),
            "fog-64": (5468, 1901), "fog-65": (4681, 2136), "fog-3000": (89995, 24113)}


@pytest.mark.parametrize("mode", ["host", "device-even", "device-odd"])
def test_walk_a_beam_set_grows_shrinks_empties(bre, synth, oracle, mode):
    """Kernel 0, counters on, 3000 bounce segments on a 1024-pixel film (zeroed per step), twelve beam sets on
    one context: 5000 -> 17 -> none -> 1 -> 20000 -> 64 -> 65 -> a third invalid -> all invalid -> per-beam
    radii (bset.uniform 0) -> one radius again -> the first set again (bit-equal to step 1).  "host" walks
    through bre_set_beams + bre_gather; the two device modes take every other step (the even or the odd ones)
    through bre_set_beams_device + bre_gather_device, so the in_* staging and the caller's arrays take turns.
    After steps 1, 5, 6 and 10 the tree is read back before the gather (tests/test_lbvh_gpu.check_tree)."""
    segs = _segs(synth, 3000)
    film0 = np.zeros((NPIX, 3), np.float32)
    opts = {bre.OPT_COUNTERS: 1}
    first = None
    with W.open_ctx(bre, opts) as g:
        for i, (name, R) in enumerate(A_STEPS):
            what = f"step {i + 1} ({name}, {mode})"
            dev = mode != "host" and i % 2 == (0 if mode == "device-even" else 1)
            beams = _beams(synth, name)
            assert beams["radius"].shape[0] <= 20000
            ref = _ref(synth, oracle, name, (3000, None), R)
            if name in A_TOTALS:
                assert (int(ref["cand"].sum()), int(ref["contrib"].sum())) == A_TOTALS[name], name
            W.set_beams(g, beams, dev)
            if i in A_TREE:
                check_tree(g, _cached(("case", name), lambda: case_of(oracle, beams)), 64, 0, has4=True)
            W.check_get_beams(bre, g, beams, dev)
            got = W.gather(g, segs, R, NPIX, film0, dev)
            with W.open_ctx(bre, opts) as f:
                W.set_beams(f, beams, dev)
                want = W.gather(f, segs, R, NPIX, film0, dev)
            W.assert_same(got, want, what)
            W.assert_oracle(got, ref, what)
            W.assert_film_composed(got, film0, segs, what)
            assert got["stats"]["n_beams"] == beams["radius"].shape[0] and got["stats"]["n_segments"] == 3000
            assert (got["stats"]["n_beams_valid"] > 0) == W.has_valid_beam(beams), what
            if not W.has_valid_beam(beams):
                assert not W.bits(got["seg_rgb"]).any() and not got["counts"].any(), what
                assert not W.bits(got["accum"]).any(), f"{what}: the film was touched"
            if i == 0:
                first = got
        for k in ("seg_rgb", "counts", "accum"):
            assert W.same_bits(got[k], first[k]), f"step 12 differs from step 1 in {k}"


# ---- walk B ----
B_COUNTS = [3000, 1, 5000, 63, 64, 65, 2, 0, 4097, 3000]


def _b_variants(bre):
    return {"default": {}, "partial-cap-1MiB": {109: 1}, "unsorted": {bre.OPT_SORT_SEGMENTS: 0},
            "kernel4-leaf8": {bre.OPT_KERNEL: 4, bre.OPT_LEAF_SIZE: 8}}


@pytest.mark.parametrize("variant", ["default", "partial-cap-1MiB", "unsorted", "kernel4-leaf8"])
def test_walk_b_segment_set_changes_on_one_build(bre, synth, oracle, variant):
    """One build of fog-5000 (R 0.01, counters on), ten gathers of 3000, 1, 5000, 63, 64, 65, 2, 0, 4097 and
    3000 segments into a 1024-pixel film: packets whose padded lanes follow a longer gather, the unsorted path
    of fewer than two segments, an empty gather (film untouched, empty outputs, n_segments 0) and the first set
    again (bit-equal).  Also with the partials capped at 1 MiB (192 segments per launch with split 256 and
    counts: 5000 segments in 27 launches, the 63 after them in one), with the segment sort off, and on kernel 4's
    tree of 8-beam leaves.  Every film is the sequential float32 compose of seg_rgb, bit for bit."""
    beams = _beams(synth, "fog-5000")
    film0 = W.film_base(NPIX)
    opts = {bre.OPT_COUNTERS: 1, **_b_variants(bre)[variant]}
    first = None
    with W.open_ctx(bre, opts) as g:
        W.set_beams(g, beams)
        for i, n in enumerate(B_COUNTS):
            what = f"step {i + 1} ({n} segments, {variant})"
            assert n <= 5000
            segs = _segs(synth, n)
            ref = _ref(synth, oracle, "fog-5000", (n, None), 0.01)
            got = W.gather(g, segs, 0.01, NPIX, film0)
            with W.open_ctx(bre, opts) as f:
                W.set_beams(f, beams)
                want = W.gather(f, segs, 0.01, NPIX, film0)
            W.assert_same(got, want, what)
            W.assert_oracle(got, ref, what)
            W.assert_film_composed(got, film0, segs, what)
            assert got["seg_rgb"].shape == (n, 3) and got["counts"].shape == (n, 2)
            assert got["stats"]["n_segments"] == n, what
            if n == 0:
                assert W.same_bits(got["accum"], film0), "an empty gather touched the film"
            if i == 0:
                first = got
        for k in ("seg_rgb", "counts", "accum"):
            assert W.same_bits(got[k], first[k]), f"the last step differs from the first in {k}"


# ---- walk C ----
def test_walk_c_kernel_changes_between_build_and_gather(bre, synth, oracle):
    """BRE_OPT_KERNEL binds twice (include/bre.h): at the build it picks the tree (kernel 0: the (start, end)
    order in BRE_OPT_TILE_LEAF-beam tiles, with the work roots and the 4-wide view made at once; 2 / 4 / 5: the
    centroid Morton order in BRE_OPT_LEAF_SIZE-beam leaves), at the gather the kernel that walks whatever tree
    is there.  All 16 (build, gather) pairs are allowed and must give the oracle's sets and sums; a kernel-0 /
    kernel-4 gather of one build gives the bits of the first such gather of that build, also after a kernel-5
    gather has reused the build's sort scratch.  One context builds with 0, 2, 4 and 5 in turn, so a tile
    kernel's roots or 4-wide view left from the previous build would walk the wrong tree."""
    beams = synth.fog_beams(3000, seed=99)  # with these segments and R: tests/test_gpu_parity.py's bounce case
    segs = synth.bounce_segments(3000, seed=5)
    R = 0.013
    ref = _cached(("ref-c",), lambda: W.oracle_ref(oracle, beams, segs, R))
    opts = {bre.OPT_COUNTERS: 1}
    with W.open_ctx(bre, opts) as g:
        for kb in (0, 2, 4, 5):
            W.set_opt(g, opts, bre.OPT_KERNEL, kb)
            W.set_beams(g, beams)
            tile_first = None
            for kg in (kb, 0, 2, 5, 4, 0):
                what = f"build with kernel {kb}, gather with kernel {kg}"
                W.set_opt(g, opts, bre.OPT_KERNEL, kg)
                got = W.gather(g, segs, R, pixel=False)
                with W.open_ctx(bre, {**opts, bre.OPT_KERNEL: kb}) as f:
                    W.set_beams(f, beams)
                    f.set_option(bre.OPT_KERNEL, kg)
                    want = W.gather(f, segs, R, pixel=False)
                # kernel 5 counts chunk candidates, not the reference's C (see the module docstring)
                W.assert_same(got, want, what, counters=kg != 5)
                W.assert_oracle(got, ref, what, cand=kg != 5)
                if kg in (0, 4):
                    if tile_first is None:
                        tile_first = got
                    assert W.same_bits(got["seg_rgb"], tile_first["seg_rgb"]), what
                    assert np.array_equal(got["counts"], tile_first["counts"]), what


# ---- walk D ----
def _expected_tree(bre, opts):
    """(leaf size, key_lo) a build under these options reports through read_tree."""
    k0 = opts.get(bre.OPT_KERNEL, 0) == 0
    leaf = opts.get(bre.OPT_TILE_LEAF, 64) if k0 else opts.get(bre.OPT_LEAF_SIZE, 1)
    return leaf, 16 if (k0 and opts.get(110, 2) >= 1 and opts.get(121, 0)) else 0


def test_walk_d_build_options_bind_at_the_build(bre, synth, oracle):
    """BRE_OPT_LEAF_SIZE (on kernel 4), BRE_OPT_TILE_LEAF, the tree order (110), the record layout (113),
    BRE_OPT_SQRT_MODE and the coarse sort keys (121), each changed after a build: the next gather walks the old
    tree (bit-identical, read_tree still reports the built leaf size and key_lo); after a rebuild read_tree
    reports the new values, and the gather meets the oracle and a fresh context.  Each option is restored and
    the set rebuilt before the next, and the restored build gives the first build's bits again."""
    beams, segs, R = _beams(synth, "fog-5000"), _segs(synth, 3000), 0.01
    film0 = W.film_base(NPIX)
    opts = {bre.OPT_COUNTERS: 1}
    cases = [(4, bre.OPT_LEAF_SIZE, 1, 8), (0, bre.OPT_TILE_LEAF, 64, 7), (0, 110, 2, 0), (0, 113, 0, 1),
             (0, bre.OPT_SQRT_MODE, 0, 1), (0, 121, 0, 1)]
    base = {}
    with W.open_ctx(bre, opts) as g:
        for kernel, opt, old, new in cases:
            what = f"option {opt} {old} -> {new} (kernel {kernel})"
            W.set_opt(g, opts, bre.OPT_KERNEL, kernel)
            W.set_opt(g, opts, opt, old)
            W.set_beams(g, beams)
            built = _expected_tree(bre, opts)
            before = W.gather(g, segs, R, NPIX, film0)
            W.assert_oracle(before, _ref(synth, oracle, "fog-5000", (3000, None), R), what + ": before")
            if kernel in base:
                W.assert_same(before, base[kernel], what + ": the restored build")
            base.setdefault(kernel, before)
            # the option alone changes nothing: the tree is the old one
            W.set_opt(g, opts, opt, new)
            after = W.gather(g, segs, R, NPIX, film0)
            W.assert_same(after, before, what + ": changed, not rebuilt")
            t = g.read_tree()
            assert (t["leaf_size"], t["key_lo"]) == built, what
            # rebuilt: the new value binds
            W.set_beams(g, beams)
            t = g.read_tree()
            assert (t["leaf_size"], t["key_lo"]) == _expected_tree(bre, opts), what
            got = W.gather(g, segs, R, NPIX, film0)
            with W.open_ctx(bre, opts) as f:
                W.set_beams(f, beams)
                want = W.gather(f, segs, R, NPIX, film0)
            W.assert_same(got, want, what + ": rebuilt")
            sq = new if opt == bre.OPT_SQRT_MODE else 0
            W.assert_oracle(got, _ref(synth, oracle, "fog-5000", (3000, None), R, sq), what + ": rebuilt")
            W.assert_film_composed(got, film0, segs, what)
            W.set_opt(g, opts, opt, old)


@pytest.mark.parametrize("counters", [True, False])
def test_walk_d_gather_options_on_one_build(bre, synth, oracle, counters):
    """One build of fog-5000, then the options the gather reads, one change per gather: BRE_OPT_SPLIT 256, 8,
    1024, 1, 256 (the roots_split cache; first and last bit-equal), BRE_OPT_PREFILTER, the segment sort key
    (105), the block map (107), the transposed-scan threshold (108), the margins (111), the tile line reject
    (112), the film by atomics and by the compose again (114: the composed film is the one before the toggle,
    bit for bit) and BRE_OPT_COUNTERS toggled and back (candidates -1 when off, contributions exact either way,
    the stats' candidates the oracle's total and not an accumulated one).  Both instantiations: counters on (the
    counting kernel) and off (the production one)."""
    beams, segs, R = _beams(synth, "fog-5000"), _segs(synth, 3000), 0.01
    ref = _ref(synth, oracle, "fog-5000", (3000, None), R)
    film0 = W.film_base(NPIX)
    opts = {bre.OPT_COUNTERS: int(counters)}
    seq = ([(bre.OPT_SPLIT, v) for v in (256, 8, 1024, 1, 256)] + [(bre.OPT_PREFILTER, 0), (bre.OPT_PREFILTER, 1)] +
           [(105, v) for v in (0, 1, 2, 3, 4)] + [(107, v) for v in (0, 1, 3)] + [(108, v) for v in (0, 4, -1)] +
           [(111, 0), (111, 1), (112, 0), (112, 1)])
    with W.open_ctx(bre, opts) as g:
        W.set_beams(g, beams)

        def step(what, film=True):
            got = W.gather(g, segs, R, NPIX, film0)
            with W.open_ctx(bre, opts) as f:
                W.set_beams(f, beams)
                want = W.gather(f, segs, R, NPIX, film0)
            on = bool(opts[bre.OPT_COUNTERS])
            W.assert_same(got, want, what, film=film, counters=on)
            W.assert_oracle(got, ref, what, counters=on)
            return got

        split = {}
        for opt, v in seq:
            W.set_opt(g, opts, opt, v)
            got = step(f"option {opt} = {v} (counters {counters})")
            W.assert_film_composed(got, film0, segs, f"option {opt} = {v}")
            if opt == bre.OPT_SPLIT:
                if v in split:
                    W.assert_same(got, split[v], "split 256 again", counters=counters)
                split[v] = got
        # every option is back at its default: the film before the toggle
        composed = got
        W.set_opt(g, opts, 114, 0)
        atomics = step("film by atomics (114 = 0)", film=False)
        assert W.same_bits(atomics["seg_rgb"], composed["seg_rgb"])
        # the same per-segment sums added to each pixel in another order: a few float32 roundings of the pixel
        # (6e-8 of its value each; at most 3 segments per pixel here), held to tests/test_gpu_parity.py's film bar
        assert W.rel_l2(atomics["accum"], composed["accum"]) <= 1e-6
        W.set_opt(g, opts, 114, 1)
        again = step("film composed again (114 = 1)")
        assert W.same_bits(again["accum"], composed["accum"]), "the composed film changed across the 114 toggle"
        # counters toggled and back
        W.set_opt(g, opts, bre.OPT_COUNTERS, int(not counters))
        other = step(f"counters {not counters}")
        W.set_opt(g, opts, bre.OPT_COUNTERS, int(counters))
        back = step(f"counters {counters} again")
        for out, on in ((other, not counters), (back, counters)):
            if on:
                assert out["stats"]["candidates"] == int(ref["cand"].sum())  # not accumulated over gathers
            else:
                assert (out["counts"][:, 0] == -1).all()
            assert np.array_equal(out["counts"][:, 1], ref["contrib"])
        assert W.same_bits(back["seg_rgb"], composed["seg_rgb"]) and W.same_bits(back["accum"], composed["accum"])


def _resolve(g, planes):
    import torch

    d = torch.from_numpy(planes).cuda().contiguous()
    img = torch.zeros((NPIX, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g.resolve_classes(d, img)
    g.synchronize()
    return img.cpu().numpy()


def test_walk_d_film_classes_and_back(bre, synth, oracle):
    """bre_gather_device on torch films: 3000 segments into one film, then 65 segments into the 8 class planes
    (the px_cls bytes of the longer, earlier order must not leak: 65 sorted segments lie in classes 0 and 1
    only), then the 3000 into one film again (bit-equal to the first).  The planes and their resolve equal a
    fresh context's bit for bit; the resolved image equals the one-film image of the same 65 segments at the bar
    tests/test_shard_gpu.py holds summed films to (relative L2 1e-6, and 1e-4 of the magnitude per bright pixel)."""
    beams, R = _beams(synth, "fog-5000"), 0.01
    big, small = _segs(synth, 3000), _segs(synth, 65)
    assert int(_ref(synth, oracle, "fog-5000", (65, None), R)["contrib"].sum()) > 0
    one0 = np.zeros((NPIX, 3), np.float32)
    planes0 = np.zeros((bre.FILM_CLASSES * NPIX, 3), np.float32)
    opts = {}

    def fresh(segs, film0):
        with W.open_ctx(bre, opts) as f:
            W.set_beams(f, beams)
            out = W.gather(f, segs, R, NPIX, film0, device=True)
            if film0 is planes0:
                out["image"] = _resolve(f, out["accum"])
        return out

    with W.open_ctx(bre, opts) as g:
        W.set_beams(g, beams)
        first = W.gather(g, big, R, NPIX, one0, device=True)
        W.assert_same(first, fresh(big, one0), "one film, 3000 segments", counters=False)
        one_small = fresh(small, one0)  # the one-film image of the 65 segments
        W.set_opt(g, opts, bre.OPT_FILM_CLASSES, bre.FILM_CLASSES)
        got = W.gather(g, small, R, NPIX, planes0, device=True)
        got["image"] = _resolve(g, got["accum"])
        want = fresh(small, planes0)
        W.assert_same(got, want, "8 class planes, 65 segments", counters=False)
        assert W.same_bits(got["image"], want["image"])
        planes = got["accum"].reshape(bre.FILM_CLASSES, NPIX, 3)
        assert planes[0].any() and not W.bits(planes[2:]).any(), "65 sorted segments lie in classes 0 and 1"
        assert W.same_bits(got["seg_rgb"], one_small["seg_rgb"])
        img, ref_img = got["image"].astype(np.float64), one_small["accum"].astype(np.float64)
        assert W.rel_l2(img, ref_img) <= 1e-6
        bright = ref_img.max(axis=1) > 1e-3 * ref_img.max()
        assert (np.abs(img - ref_img)[bright] <= 1e-4 * np.abs(ref_img[bright]).max(axis=1, keepdims=True)).all()
        W.set_opt(g, opts, bre.OPT_FILM_CLASSES, 1)
        last = W.gather(g, big, R, NPIX, one0, device=True)
        W.assert_same(last, first, "one film again", counters=False)
        W.assert_film_composed(last, one0, big, "one film again")


def test_walk_d_packet_shards_and_back(bre, synth):
    """set_shard(r, 2, packets=True) for r = 0, then 1, on one context, then one shard again: each shard equals
    a fresh context's; a shard's own entries (C = -1, counters off) carry the unsharded bits and the rest are
    zero, every segment owned once (the bar of test_packet_shard_outputs_are_defined_and_sum); the two films sum
    to the unsharded one to float summation order (relative L2 1e-6); the final unsharded gather is the first,
    bit for bit."""
    beams, segs, R = _beams(synth, "fog-5000"), _segs(synth, 3000), 0.01
    film0 = np.zeros((NPIX, 3), np.float32)
    opts = {}

    def shard(g, rank, count, packets):
        for k, v in ((bre.OPT_SHARD_MODE, int(packets)), (bre.OPT_SHARD_BLOCK, 1), (bre.OPT_SHARD_COUNT, count),
                     (bre.OPT_SHARD_RANK, rank)):  # BeamGather.set_shard's order
            W.set_opt(g, opts, k, v)

    def fresh():
        with W.open_ctx(bre, opts) as f:
            W.set_beams(f, beams)
            return W.gather(f, segs, R, NPIX, film0, device=True)

    with W.open_ctx(bre, opts) as g:
        W.set_beams(g, beams)
        whole = W.gather(g, segs, R, NPIX, film0, device=True)
        W.assert_same(whole, fresh(), "unsharded", counters=False)
        assert whole["seg_rgb"].any()
        owned = np.zeros(3000, np.int32)
        parts = []
        for r in (0, 1):
            shard(g, r, 2, True)
            got = W.gather(g, segs, R, NPIX, film0, device=True)
            W.assert_same(got, fresh(), f"packet shard {r} of 2", counters=False)
            assert got["stats"]["n_segments"] == bre.shard_segments(3000, r, 2, 1)
            mine = got["counts"][:, 0] == -1
            owned += mine
            assert not W.bits(got["seg_rgb"][~mine]).any() and not got["counts"][~mine].any()
            assert W.same_bits(got["seg_rgb"][mine], whole["seg_rgb"][mine])
            assert np.array_equal(got["counts"][mine], whole["counts"][mine])
            parts.append(got["accum"].astype(np.float64))
        assert (owned == 1).all()
        assert W.rel_l2(parts[0] + parts[1], whole["accum"]) <= 1e-6
        shard(g, 0, 1, False)
        last = W.gather(g, segs, R, NPIX, film0, device=True)
        W.assert_same(last, whole, "unsharded again", counters=False)


# ---- walk E ----
PHOTONS, DEPTH, R_PASS = 20000, 5, 0.02


def _passes(g, s, w, h, it):
    """trace_photons + camera_pass + gather_camera_segments on g: everything the three calls leave behind."""
    import torch

    surf = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    film = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    nb = g.trace_photons(s, PHOTONS, iteration=it, max_depth=DEPTH, radius=R_PASS)
    ns = g.camera_pass(s, w, h, iteration=it, max_depth=DEPTH, surface=surf)
    rgb = torch.zeros((ns, 3), dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    g.gather_camera_segments(R_PASS, accum=film, seg_rgb=rgb)
    g.synchronize()
    out = {"beams": g.get_beams(), "segs": g.get_segments(), "surface": surf.cpu().numpy(), "film": film.cpu().numpy(),
           "seg_rgb": rgb.cpu().numpy(), "stats": g.stats()}
    assert nb == out["beams"]["radius"].shape[0] and ns == out["segs"]["tmax"].shape[0]
    return out


def _assert_passes_same(got, want, what):
    for k in W.BEAM_KEYS:
        assert W.same_bits(got["beams"][k], want["beams"][k]), f"{what}: beams {k} differ from a fresh context's"
    for k in ("o", "p", "d", "tmax", "pixel", "depth"):
        assert W.same_bits(got["segs"][k], want["segs"][k]), f"{what}: segments {k} differ from a fresh context's"
    for k in ("surface", "film", "seg_rgb"):
        assert W.same_bits(got[k], want[k]), f"{what}: {k} differs from a fresh context's"
    for k in W.STAT_KEYS + ("n_photons", "n_camera_segments"):
        assert got["stats"][k] == want["stats"][k], (what, k)


def _moved_vertex(scene_mod):
    s = scene_mod.cornell_scene()
    assert not s.triangles[4].emit  # the back wall
    s.triangles[4].p[0][2] += 1.0 / 64
    return s


def test_walk_e_scene_medium_and_film_caches(bre, oracle, scene_mod_gpu):
    """The Cornell box in fog (as tests/test_photon_gpu.py and tests/test_camera_gpu.py build it), 20000 photons,
    max_depth 5, films of 32x32 and 48x16, the three passes per step on one context: the same scene twice (every
    cache hits), the medium's sigma_s alone (ph_scene_host misses), one wall vertex moved by 1/64 (sc_hash
    misses), the first scene again, grid media (one density value changed with the dimensions kept: grid_bytes
    misses; the dimensions permuted with the values kept), the film size there and back, the camera alone, and
    iteration 0 -> 3 -> 0.  Beams, segments, surface film, per-segment sums and gathered film equal a fresh
    context's bit for bit at every step; the oracle's photon and camera passes are matched bit for bit where
    the step list says so."""
    sm = scene_mod_gpu
    plain = sm.cornell_scene()
    dens5 = sm.smoke_density(5, 7)
    dens5b = dens5.copy()
    dens5b[60] += np.float32(0.25)
    rng = np.random.default_rng(11)
    dens456 = rng.random(120).astype(np.float32)
    cam = sm.cornell_scene()
    cam.cam_pos = sm.F3(0.45, 0.5, 0.02)
    thick = lambda d, n: sm.grid_medium(sm.cornell_scene(1.0, 1.0, 0.0), d, n)  # noqa: E731
    # (what, scene, width, height, iteration, also against the oracle)
    steps = [("1 the scene", plain, 32, 32, 0, True),
             ("2 the same scene", sm.cornell_scene(), 32, 32, 0, True),
             ("3 sigma_s alone", sm.cornell_scene(sigma_s=0.7), 32, 32, 0, True),
             ("4 one vertex moved", _moved_vertex(sm), 32, 32, 0, True),
             ("5 the first scene again", plain, 32, 32, 0, False),
             ("6a grid medium", sm.cornell_smoke_scene(sigma_a=1.0, sigma_s=1.0, g=0.0, n=5), 32, 32, 0, False),
             ("6b one density value", thick(dens5b, 5), 32, 32, 0, False),
             ("6c a 4x5x6 grid", thick(dens456, (4, 5, 6)), 32, 32, 0, False),
             ("6d the same values as 6x5x4", thick(dens456, (6, 5, 4)), 32, 32, 0, False),
             ("7a film 32x32", plain, 32, 32, 0, False), ("7b film 48x16", plain, 48, 16, 0, False),
             ("7c film 32x32 again", plain, 32, 32, 0, False), ("7d the camera alone", cam, 32, 32, 0, False),
             ("8a iteration 0", plain, 32, 32, 0, True), ("8b iteration 3", plain, 32, 32, 3, True),
             ("8c iteration 0 again", plain, 32, 32, 0, True)]
    seen = {}
    with bre.BeamGather(0) as g:
        for what, s, w, h, it, vs_oracle in steps:
            assert w * h <= 48 * 48
            got = _passes(g, s, w, h, it)
            with bre.BeamGather(0) as f:
                want = _passes(f, s, w, h, it)
            _assert_passes_same(got, want, what)
            assert got["beams"]["radius"].shape[0] > 0 and got["film"].any(), what
            if vs_oracle:
                key = ("passes", s.to_bytes(), w, h, it)
                ob, oc = _cached(key, lambda: (oracle.trace_photons(s, PHOTONS, iteration=it, max_depth=DEPTH,
                                                                    radius=R_PASS),
                                               oracle.camera_pass(s, w, h, iteration=it, max_depth=DEPTH)))
                _assert_beams_equal(got["beams"], ob)
                _assert_segments_equal(got["segs"], oc)
                assert W.same_bits(got["surface"], oc["surface"]), what
            seen[what] = got
        _assert_passes_same(seen["5 the first scene again"], seen["1 the scene"], "step 5 against step 1")
        _assert_passes_same(seen["7c film 32x32 again"], seen["1 the scene"], "step 7c against step 1")
        _assert_passes_same(seen["8c iteration 0 again"], seen["8a iteration 0"], "step 8c against step 8a")
        # the steps that must differ do (a cache that never missed would pass everything above otherwise)
        for a, b in (("3 sigma_s alone", "1 the scene"), ("4 one vertex moved", "1 the scene"),
                     ("6b one density value", "6a grid medium"), ("6d the same values as 6x5x4", "6c a 4x5x6 grid"),
                     ("7d the camera alone", "7c film 32x32 again"), ("8b iteration 3", "8a iteration 0")):
            assert not W.same_bits(seen[a]["film"], seen[b]["film"]), f"{a} gave the film of {b}"


def test_walk_e_external_triangles_mutated_in_place(bre, oracle, scene_mod_gpu):
    """A scene past the inline triangles (triangles_ext): the caller moves a vertex in its own array between two
    calls, so the bre_scene bytes are the same; the geometry must follow the contents (upload_scene compares the
    triangles' bytes), as a fresh context and the oracle see them."""
    sm = scene_mod_gpu
    s = sm.cornell_sphere_scene(n_theta=8, n_phi=12)
    assert s.n_triangles > sm.MAX_TRIANGLES and s.triangles_ext
    films = []
    tri = s._triangles_ref[20]  # a triangle of the sphere
    assert not tri.emit
    y0 = float(tri.p[0][1])
    head = s.to_bytes()
    with bre.BeamGather(0) as g:
        for y in (y0, y0 + 1.0 / 64, y0):
            tri.p[0][1] = y
            assert s.to_bytes() == head  # only the external array changed
            got = _passes(g, s, 32, 32, 0)
            with bre.BeamGather(0) as f:
                want = _passes(f, s, 32, 32, 0)
            _assert_passes_same(got, want, f"external triangles, vertex y = {y}")
            _assert_beams_equal(got["beams"], oracle.trace_photons(s, PHOTONS, iteration=0, max_depth=DEPTH,
                                                                   radius=R_PASS))
            films.append(got)
    assert not W.same_bits(films[0]["beams"]["end"], films[1]["beams"]["end"]), "the moved vertex changed nothing"
    _assert_passes_same(films[2], films[0], "moved back")


# ---- walk F ----
def test_walk_f_refused_calls_leave_the_context_as_it_was(bre, synth, oracle, scene_mod_gpu):
    """A good build (fog-20000) and gather, then one refused call after another, each with its status, and the
    good gather again after each: bit-equal to the first every time.  A device error flag is reported exactly
    once (the call after it succeeds)."""
    import torch

    beams, segs, R = _beams(synth, "fog-20000"), _segs(synth, 3000), 0.01
    ref = _ref(synth, oracle, "fog-20000", (3000, None), R)
    film0 = W.film_base(NPIX)
    opts = {bre.OPT_COUNTERS: 1}
    bad = {k: v.copy() for k, v in segs.items()}
    bad["pixel"][7] = NPIX  # out of [0, npix)
    dark = scene_mod_gpu.cornell_scene()
    dark.triangles[12].emit = dark.triangles[13].emit = 0  # no area light

    def refused(status, call, *a, **kw):
        with pytest.raises(bre.BreError) as e:
            call(*a, **kw)
        assert e.value.status == status, (e.value.status, str(e.value))

    with W.open_ctx(bre, opts) as g:
        W.set_beams(g, beams)
        first = W.gather(g, segs, R, NPIX, film0)
        W.assert_oracle(first, ref, "the good gather")

        def good(what, device=False):
            again = W.gather(g, segs, R, NPIX, film0, device)
            W.assert_same(again, first, what)
            W.check_get_beams(bre, g, beams, False)

        null = [None] * 4
        refused(W.BRE_ERR_INVALID_ARG, lambda: g._check(g.lib.bre_set_beams(g.h, -1, *null)))
        good("after bre_set_beams with a negative count")
        refused(W.BRE_ERR_INVALID_ARG, lambda: g._check(g.lib.bre_set_beams(g.h, 5, *null)))
        good("after bre_set_beams with null arrays")
        refused(W.BRE_ERR_INVALID_ARG, g.set_option, bre.OPT_SPLIT, 3)
        refused(W.BRE_ERR_INVALID_ARG, g.set_option, bre.OPT_KERNEL, 1)
        good("after out-of-range options")
        # a pixel out of range: at the call for the host entry
        refused(W.BRE_ERR_INVALID_ARG, W.gather, g, bad, R, NPIX, film0)
        good("after a bad pixel through bre_gather")
        # ... and at synchronize() for the device entry, once
        d = {k: torch.from_numpy(v).cuda().contiguous() for k, v in bad.items()}
        acc = torch.zeros((NPIX, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        g.gather_device(d["o"], d["p"], d["d"], d["tmax"], d["pixel"], R, NPIX, accum=acc)
        refused(W.BRE_ERR_INVALID_ARG, g.synchronize)
        g.synchronize()  # reported once
        good("after a bad pixel through bre_gather_device", device=True)
        good("the host entry after the device entry")
        # a traversal-stack overflow (internal option 101, one work root so that the walk needs its stack)
        g.set_option(bre.OPT_SPLIT, 1)
        g.set_option(101, 2)
        refused(W.BRE_ERR_STATE, W.gather, g, segs, R, NPIX, film0)
        g.synchronize()  # reported once
        g.set_option(101, 0)
        g.set_option(bre.OPT_SPLIT, 256)
        good("after a traversal-stack overflow")
        # a scene with no light: refused before the beam set is touched
        refused(W.BRE_ERR_INVALID_ARG, g.trace_photons, dark, 1000)
        good("after trace_photons on a scene with no light")
        # read_tree after a kernel-5 gather has reused the build's sort scratch
        g.set_option(bre.OPT_KERNEL, 5)
        k5 = W.gather(g, segs, R, NPIX, None)
        W.assert_oracle(k5, ref, "the kernel-5 gather", cand=False)
        refused(W.BRE_ERR_STATE, g.read_tree)
        g.set_option(bre.OPT_KERNEL, 0)
        good("after a refused read_tree")
        W.set_beams(g, beams)
        t = g.read_tree()
        assert t["nvalid"] == 20000 and (t["leaf_size"], t["key_lo"]) == (64, 0) and t["nodes4"] is not None
        good("after the rebuild")
