"""The tile kernel's specialised production instantiation gives the generic instantiation's bits.

k_gather_tile<false, 6, TileProd> (bre_gather.hip) states the options every default context binds as
template constants: prefilter on, margin mode 1, the LPT block map, 64-beam leaves, a tile-axis table,
no contribution counts, a uniform-radius set.  launch_gather_tile picks it per launch when the bound
options and the beam set match; internal option 123 = 0 forces the generic instantiation, and
bre_stats.tile_variant reports which one the last gather launched (1 generic, 2 specialised).

Every case gathers the same segments with option 123 = 1 and 0 and compares the per-segment sums bit
for bit, and with per-segment counts (which both run through the generic instantiation: the
specialisation has no counting form) the counts, the sums again and the exact stage's queue length.
The cases reach the rare paths the specialisation must keep: a last packet with one valid lane, fewer
beams than one tile and fewer work roots than S, a segment repeated more than 8 times in one exact
batch (the rounds loop behind the transposed scan) with a partial final batch, an axis-parallel ray, a
zero-length segment, a zero-length beam, and a MaxDistance for each transposed-scan threshold."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GENERIC, SPECIALISED = 1, 2
OPT_TILE_SPEC = 123


def _set_beams(g, beams):
    g.set_beams(beams["start"], beams["end"], beams["radius"], beams["power"])


def _gather(bre, beams, segs, R, spec, counts=False, options=(), timing=False):
    """One gather on a fresh context: (outputs, stats).  `options`: (option, value) pairs set before the build."""
    with bre.BeamGather(0, timing=timing) as g:
        g.set_option(OPT_TILE_SPEC, spec)
        for k, v in options:
            g.set_option(k, v)
        _set_beams(g, beams)
        out = g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], R=R, counts=counts)
        return out, g.stats()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check_pair(bre, beams, segs, R, options=()):
    """Option 123 = 1 against 0 on one workload; returns the counting run's outputs and stats."""
    spec, st1 = _gather(bre, beams, segs, R, 1, options=options)
    gen, st0 = _gather(bre, beams, segs, R, 0, options=options)
    assert st1["tile_variant"] == SPECIALISED
    assert st0["tile_variant"] == GENERIC
    assert np.array_equal(_bits(spec["seg_rgb"]), _bits(gen["seg_rgb"]))
    # with counts both contexts launch the generic instantiation: same counts, queue length and sums
    c1, sc1 = _gather(bre, beams, segs, R, 1, counts=True, options=options, timing=True)
    c0, sc0 = _gather(bre, beams, segs, R, 0, counts=True, options=options, timing=True)
    assert sc1["tile_variant"] == GENERIC and sc0["tile_variant"] == GENERIC
    assert np.array_equal(c1["counts"], c0["counts"])
    assert sc1["queued_pairs"] == sc0["queued_pairs"]
    assert np.array_equal(_bits(c1["seg_rgb"]), _bits(c0["seg_rgb"]))
    assert np.array_equal(_bits(c1["seg_rgb"]), _bits(spec["seg_rgb"]))
    return c1, sc1


def _rare_segments(synth, n, seed):
    """n incoherent segments with one axis-parallel ray (infinite 1/d on two axes) and one zero-length one."""
    segs = synth.bounce_segments(n, seed=seed)
    segs["d"][7] = np.array([0.0, 0.0, 1.0], np.float32)
    segs["p"][7] = segs["o"][7] + segs["tmax"][7] * segs["d"][7]
    segs["p"][11] = segs["o"][11]
    segs["tmax"][11] = 0.0
    return segs


# MaxDistance = R + radius picks the transposed-scan threshold (tscan_for, bre_api_gather.hip):
# >= 0.015: 3, >= 0.008: 4, below: 5
@pytest.mark.parametrize("radius,R,tscan", [(0.01, 0.01, 3), (0.004, 0.005, 4), (0.002, 0.003, 5)])
def test_specialised_matches_generic(bre, synth, radius, R, tscan):
    maxd = np.float32(R) + np.float32(radius)
    assert (3 if maxd >= 0.015 else 4 if maxd >= 0.008 else 5) == tscan
    beams = synth.fog_beams(4000, seed=301, radius=radius)
    beams["end"][5] = beams["start"][5]  # a zero-length beam: NaN box, never gathered
    segs = _rare_segments(synth, 5 * 64 + 1, seed=302)  # the last packet has exactly one valid lane
    out, st = _check_pair(bre, beams, segs, R)
    assert st["n_beams_valid"] == 3999
    assert out["counts"][:, 1].sum() > 0
    assert (out["counts"][:, 0] == -1).all()  # the production control flow: candidates are not counted


def test_fewer_beams_than_a_tile(bre, synth):
    """nb < 64: one leaf tile, a tree with one work root where S = 256."""
    beams = synth.fog_beams(40, seed=311, radius=0.03, mean_length=0.7)
    segs = _rare_segments(synth, 2 * 64 + 2, seed=312)
    out, _ = _check_pair(bre, beams, segs, 0.04)
    assert out["counts"][:, 1].sum() > 0


def test_one_segment_many_rounds(bre, synth):
    """One segment (a packet with one valid lane) in a dense set on one work root: every queued pair is
    that segment's, so a batch of 64 holds as many read-modify-write rounds as it has contributing pairs.
    More contributions than 8 per batch means some batch went past the eight unrolled rounds, and a queue
    length that is no multiple of 64 ends in a partial batch."""
    beams = synth.fog_beams(6000, seed=321, radius=0.03, mean_length=0.7)
    many = synth.bounce_segments(64, seed=322)
    i = int(np.argmax(many["tmax"]))  # the longest one
    segs = {k: v[i:i + 1].copy() for k, v in many.items()}
    opts = ((bre.OPT_SPLIT, 1),)
    out, st = _check_pair(bre, beams, segs, 0.04, options=opts)
    batches = (st["queued_pairs"] + 63) // 64
    assert out["counts"][0, 1] > 8 * batches
    assert st["queued_pairs"] % 64 != 0


def test_dense_packets(bre, synth):
    """Dense incoherent packets (transposed tiles: long stretches of one segment per batch)."""
    beams = synth.fog_beams(5000, seed=331, radius=0.03, mean_length=0.7)
    segs = _rare_segments(synth, 3 * 64 + 17, seed=332)
    out, st = _check_pair(bre, beams, segs, 0.04)
    assert out["counts"][:, 1].max() > 64
    assert st["queued_pairs"] % 64 != 0


@pytest.mark.parametrize("what", ["mixed_radius", "margin0", "prefilter_off", "no_tile_axis", "tile_leaf_32",
                                  "occupancy_7", "block_map_1"])
def test_other_settings_run_the_generic_instantiation(bre, synth, what):
    """Only the reported instantiation: the results of these settings are the existing option tests'."""
    beams = synth.fog_beams(2000, seed=341, radius=0.01)
    options = {"mixed_radius": (), "margin0": ((111, 0),), "prefilter_off": ((bre.OPT_PREFILTER, 0),),
               "no_tile_axis": ((112, 0),), "tile_leaf_32": ((bre.OPT_TILE_LEAF, 32),), "occupancy_7": ((102, 7),),
               "block_map_1": ((107, 1),)}[what]
    if what == "mixed_radius":
        beams["radius"][::2] = np.float32(0.02)
    segs = synth.bounce_segments(200, seed=342)
    _, st = _gather(bre, beams, segs, 0.01, 1, options=options)
    assert st["tile_variant"] == GENERIC


def _pipelined_film(bre, scene, spec, iters, w, h, photons):
    """iters rendered alternately by two linked contexts (bre_set_gather_after) through bre_gather_camera."""
    import torch

    film = torch.zeros((w * h, 3), dtype=torch.float32, device="cuda")
    parts = [torch.zeros_like(film), torch.zeros_like(film)]
    surf = [torch.zeros_like(film), torch.zeros_like(film)]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    ctxs = [bre.BeamGather(0), bre.BeamGather(0)]
    variants = []
    try:
        for g, st in zip(ctxs, streams):
            g.set_option(OPT_TILE_SPEC, spec)
            g.set_stream(st.cuda_stream)
        ctxs[0].set_gather_after(ctxs[1])
        ctxs[1].set_gather_after(ctxs[0])
        done = [None, None]
        for k, it in enumerate(iters):
            i = k % 2
            g, st = ctxs[i], streams[i]
            with torch.cuda.stream(st):
                if k >= 1:  # the film adds happen in iteration order
                    st.wait_event(done[1 - i])
                R = bre.beam_radius_at(0.05, 0.5, it)
                g.trace_photons(scene, photons, it, 5, R)
                g.camera_pass(scene, w, h, it, 5, True, True, surface=surf[i])
                g.gather_camera(R, parts[i])
                variants.append(g.stats()["tile_variant"])
                g.film_add(parts[i], film, clear_src=True)
                done[i] = torch.cuda.Event()
                done[i].record(st)
        torch.cuda.synchronize()
    finally:
        ctxs[1].set_gather_after(None)
        for g in ctxs:
            g.close()
    return film.cpu().numpy(), variants


def test_pipelined_render_film(bre, scene_mod_gpu):
    """32 x 32 render iterations on two pipelined contexts: film against film."""
    scene = scene_mod_gpu.cornell_scene(0.05, 0.5, 0.0)
    iters = [0, 1]
    film1, v1 = _pipelined_film(bre, scene, 1, iters, 32, 32, 5000)
    film0, v0 = _pipelined_film(bre, scene, 0, iters, 32, 32, 5000)
    assert v1 == [SPECIALISED] * len(iters) and v0 == [GENERIC] * len(iters)
    assert np.abs(film1).sum() > 0
    assert np.array_equal(_bits(film1), _bits(film0))
