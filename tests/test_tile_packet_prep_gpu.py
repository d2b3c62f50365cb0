"""The packet record of the specialised tile kernel gives the generic instantiation's bits.

k_packet_prep (bre_gather.hip) forms each 64-segment packet's bundle and largest lane margin once per launch
(PacketRec, bre_packet.h) with make_bundle and make_scan_lane themselves; k_gather_tile<false, 7, TileProd> reads
its packet's record with scalar loads instead of forming the bundle in every (packet, work root) wave, and takes
1 / MaxDistance from the host.  The generic instantiation (internal option 123 = 0) still forms the bundle in the
kernel.

Every case gathers the same segments with option 123 = 1 and 0 on fresh contexts and compares the per-segment
sums bit for bit; with per-segment counts (the generic instantiation at either setting) the counts, the exact
stage's queue length and the sums again.  bre_device_check kind 15 forms the records again in a wave per packet
and compares the stored ones word for word.  The shapes are the small ones at which the change can go wrong: whole
and ragged last packets for each transposed-scan threshold, a packet of zero-length segments (bundle disabled by
its margin), an axis-parallel ray, coincident origins, fewer beams than a tile, a transposed tile with a drain
between two of its steps, fixed thresholds against the default, packet shards (records numbered within the
shard's launch), several launches per gather, one context through a resize up and down, and two pipelined
contexts film against film."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GENERIC, SPECIALISED = 1, 2
OPT_TSCAN, OPT_PARTIAL_MIB, OPT_TILE_SPEC = 108, 109, 123
KIND_PACKET_RECORDS = 15


def _ctx(bre, spec, options=(), counts=False):
    g = bre.BeamGather(0, timing=counts)
    g.set_option(OPT_TILE_SPEC, spec)
    for k, v in options:
        g.set_option(k, v)
    return g


def _gather(bre, beams, segs, R, spec, counts=False, options=()):
    with _ctx(bre, spec, options, counts) as g:
        g.set_beams(beams["start"], beams["end"], beams["radius"], beams["power"])
        out = g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], R=R, counts=counts)
        return out, g.stats()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _check(bre, beams, segs, R, options=()):
    """Specialised against generic on one workload; returns a counting run's outputs and stats."""
    a, sa = _gather(bre, beams, segs, R, 1, options=options)
    b, sb = _gather(bre, beams, segs, R, 0, options=options)
    assert sa["tile_variant"] == SPECIALISED and sb["tile_variant"] == GENERIC
    assert np.array_equal(_bits(a["seg_rgb"]), _bits(b["seg_rgb"]))
    c1, s1 = _gather(bre, beams, segs, R, 1, counts=True, options=options)
    c0, s0 = _gather(bre, beams, segs, R, 0, counts=True, options=options)
    assert s1["tile_variant"] == GENERIC and s0["tile_variant"] == GENERIC
    assert np.array_equal(c1["counts"], c0["counts"])
    assert s1["queued_pairs"] == s0["queued_pairs"]
    assert np.array_equal(_bits(c1["seg_rgb"]), _bits(c0["seg_rgb"]))
    assert np.array_equal(_bits(c1["seg_rgb"]), _bits(a["seg_rgb"]))
    return c1, s1


def _rare_segments(synth, n, seed):
    """n incoherent segments with one axis-parallel ray (infinite 1/d on two axes) and one zero-length one."""
    segs = synth.bounce_segments(n, seed=seed)
    segs["d"][7] = np.array([0.0, 0.0, 1.0], np.float32)
    segs["p"][7] = segs["o"][7] + segs["tmax"][7] * segs["d"][7]
    segs["p"][11] = segs["o"][11]
    segs["tmax"][11] = 0.0
    return segs


@pytest.fixture(scope="module")
def fog(synth):
    return {r: synth.fog_beams(4000, seed=501, radius=r) for r in (0.01, 0.004, 0.002)}


@pytest.fixture(scope="module")
def dense(synth):
    return synth.fog_beams(5000, seed=541, radius=0.03, mean_length=0.7)


# MaxDistance = R + radius picks the base transposed-scan threshold (tscan_for, bre_api_gather.hip):
# >= 0.015: 3, >= 0.008: 4, below: 5
@pytest.mark.parametrize("nseg", [64, 65, 129])
@pytest.mark.parametrize("radius,R,tscan", [(0.01, 0.01, 3), (0.004, 0.005, 4), (0.002, 0.003, 5)])
def test_whole_and_ragged_packets(bre, synth, fog, radius, R, tscan, nseg):
    maxd = np.float32(R) + np.float32(radius)
    assert (3 if maxd >= 0.015 else 4 if maxd >= 0.008 else 5) == tscan
    segs = _rare_segments(synth, nseg, seed=502)  # 65, 129: one valid lane beside 63 unwritten records
    out, _ = _check(bre, fog[radius], segs, R)
    assert out["counts"][:, 1].sum() > 0


def test_packet_of_zero_length_segments(bre, synth, dense):
    """Every lane's Al' is FLT_MAX: al_max is 0, the bundle line falls back, nothing may be rejected wrongly."""
    segs = synth.bounce_segments(64, seed=511)
    segs["p"][:] = segs["o"]
    segs["tmax"][:] = 0.0
    _check(bre, dense, segs, 0.04)


def test_packet_with_one_axis_parallel_ray(bre, synth, dense):
    segs = synth.bounce_segments(64, seed=512)
    segs["d"][5] = np.array([0.0, 1.0, 0.0], np.float32)
    segs["p"][5] = segs["o"][5] + segs["tmax"][5] * segs["d"][5]
    out, _ = _check(bre, dense, segs, 0.04)
    assert out["counts"][:, 1].sum() > 0


def test_packet_of_coincident_origins(bre, synth, dense):
    """The primary-ray case: every origin is the same point, so delta comes from the end points alone."""
    segs = synth.bounce_segments(70, seed=513)
    o = np.array([0.5, 0.5, -0.9], np.float32)
    v = segs["p"] - o
    t = np.sqrt((v.astype(np.float64) ** 2).sum(1)).astype(np.float32)
    segs["o"][:] = o
    segs["d"][:] = v / t[:, None]
    segs["tmax"][:] = t
    out, _ = _check(bre, dense, segs, 0.04)
    assert out["counts"][:, 1].sum() > 0


def test_fewer_beams_than_a_tile(bre, synth):
    beams = synth.fog_beams(40, seed=521, radius=0.03, mean_length=0.7)
    out, _ = _check(bre, beams, _rare_segments(synth, 2 * 64 + 1, seed=522), 0.04)
    assert out["counts"][:, 1].sum() > 0


def test_drain_between_two_steps_of_a_transposed_tile(bre, synth):
    """Three segments on one work root with a MaxDistance that covers the scene, the threshold forced to 8: a tile
    with more than three kept beams goes transposed in two steps, lanes 0 and 1, then lane 2.  The queue holds
    fewer than 64 pairs before any step.  A tile's last step adds at most 64 (one lane), so the drain after it runs
    at most one batch; a beam-major tile (at most three kept beams, nine pairs) runs at most one in all.  More
    full batches than tiles therefore means that the exact stage ran between the two steps of some transposed tile,
    whose second step then works with the queue moved."""
    beams = synth.fog_beams(2000, seed=531, radius=0.03, mean_length=0.7)
    many = synth.bounce_segments(64, seed=532)
    top = np.argsort(many["tmax"])[-3:]
    segs = {k: v[top].copy() for k, v in many.items()}
    out, st = _check(bre, beams, segs, 1.0, options=((bre.OPT_SPLIT, 1), (OPT_TSCAN, 8)))
    tiles = (2000 + 63) // 64
    print("queued pairs", st["queued_pairs"], "tiles", tiles)
    assert st["queued_pairs"] // 64 > tiles
    assert out["counts"][:, 1].max() > 64


def test_dense_packets(bre, synth, dense):
    """Dense incoherent packets: transposed tiles with many lanes on, long stretches of one segment per batch."""
    out, st = _check(bre, dense, _rare_segments(synth, 3 * 64 + 17, seed=542), 0.04)
    assert out["counts"][:, 1].max() > 64
    assert st["queued_pairs"] % 64 != 0


@pytest.mark.parametrize("t", [0, 3, 8])
def test_fixed_threshold_against_the_default(bre, synth, dense, t):
    """Option 108 >= 0 forces the threshold; the sums are the default's bits for any threshold."""
    segs = _rare_segments(synth, 64 + 30, seed=551)
    want, _ = _gather(bre, dense, segs, 0.04, 1)
    for spec in (1, 0):
        got, st = _gather(bre, dense, segs, 0.04, spec, options=((OPT_TSCAN, t),))
        assert st["tile_variant"] == (SPECIALISED if spec else GENERIC)
        assert np.array_equal(_bits(got["seg_rgb"]), _bits(want["seg_rgb"]))


def test_packet_shards_number_their_own_records(bre, synth, dense):
    """Shards 1/2 and 2/2 of 200 segments: each gathers its own packets renumbered from 0; the two outputs (zero
    for the other shard's segments) add up to the unsharded sums."""
    segs = _rare_segments(synth, 200, seed=561)
    whole, _ = _gather(bre, dense, segs, 0.04, 1)
    for spec in (1, 0):
        parts = []
        for rank in (0, 1):
            with _ctx(bre, spec) as g:
                g.set_shard(rank, 2, 1, packets=True)
                g.set_beams(dense["start"], dense["end"], dense["radius"], dense["power"])
                parts.append(g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], R=0.04)["seg_rgb"])
                assert g.stats()["tile_variant"] == (SPECIALISED if spec else GENERIC)
        assert parts[0].any() and parts[1].any()
        assert not (parts[0].any(axis=1) & parts[1].any(axis=1)).any()
        assert np.array_equal(parts[0] + parts[1], whole["seg_rgb"])


def test_two_launches_per_gather(bre, synth, dense):
    """Option 109 at 1 MiB: S = 256 partial sums of 12 B per segment allow 320 segments per launch, so 400 take two;
    the second launch's records are numbered from 0 again."""
    segs = _rare_segments(synth, 400, seed=571)
    want, _ = _gather(bre, dense, segs, 0.04, 1)
    for spec in (1, 0):
        got, st = _gather(bre, dense, segs, 0.04, spec, options=((OPT_PARTIAL_MIB, 1),))
        assert st["tile_variant"] == (SPECIALISED if spec else GENERIC)
        assert np.array_equal(_bits(got["seg_rgb"]), _bits(want["seg_rgb"]))


def test_one_context_through_resizes(bre, synth, dense):
    """65, then 4,000, then 65 segments on one long-lived context: the record buffer grows with the segment
    records and is reused after it."""
    sets = [_rare_segments(synth, n, seed=580 + i) for i, n in enumerate((65, 4000, 65))]
    with _ctx(bre, 1) as g:
        g.set_beams(dense["start"], dense["end"], dense["radius"], dense["power"])
        got = []
        for s in sets:
            got.append(g.gather(s["o"], s["p"], s["d"], s["tmax"], R=0.04)["seg_rgb"])
            assert g.stats()["tile_variant"] == SPECIALISED
    with _ctx(bre, 0) as g:
        g.set_beams(dense["start"], dense["end"], dense["radius"], dense["power"])
        for s, a in zip(sets, got):
            b = g.gather(s["o"], s["p"], s["d"], s["tmax"], R=0.04)["seg_rgb"]
            assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("nseg", [65, 129])
def test_stored_records_word_for_word(bre, synth, dense, nseg):
    """bre_device_check kind 15 on the records a gather in the caller's order left in the context."""
    segs = _rare_segments(synth, nseg, seed=590)
    x = np.concatenate([segs["o"], segs["p"], segs["d"], segs["tmax"][:, None]], axis=1).astype(np.float32)
    with _ctx(bre, 1, options=((bre.OPT_SORT_SEGMENTS, 0),)) as g:
        g.set_beams(dense["start"], dense["end"], dense["radius"], dense["power"])
        g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], R=0.04)
        assert g.stats()["tile_variant"] == SPECIALISED
        y = g.device_check(KIND_PACKET_RECORDS, x.ravel())
        assert y[0] == 0 and y[1] == (nseg + 63) // 64
        # the check does see a difference: another end point for one segment of the last packet moves its bundle
        x2 = x.copy()
        x2[nseg - 1, 3:6] += np.float32(0.25)
        assert g.device_check(KIND_PACKET_RECORDS, x2.ravel())[0] > 0
        # and it refuses segments that are not the last launch's
        with pytest.raises(bre.BreError, match="kind 15"):
            g.device_check(KIND_PACKET_RECORDS, x[:-1].ravel())


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
    """Two 32 x 32 render iterations on two pipelined contexts: film against film."""
    scene = scene_mod_gpu.cornell_scene(0.05, 0.5, 0.0)
    films = {}
    for spec in (1, 0):
        films[spec], v = _pipelined_film(bre, scene, spec, [0, 1], 32, 32, 5000)
        assert v == [SPECIALISED if spec else GENERIC] * 2
    assert np.abs(films[1]).sum() > 0
    assert np.array_equal(_bits(films[1]), _bits(films[0]))
