"""The whole render on several contexts (bre_render_sharded, bre_render_progressive_sharded; here all on
GPU 0) and the film collective behind it and behind bre_gather_sharded.

The expected images are built only from the single-context entry points (trace_photons, camera_pass,
gather_camera on films of the test's own, bre_resolve_image, bre_render, bre_gather), never from the
sharded calls:

* recipe A (class planes), per rank r of n: a context with BRE_OPT_FILM_CLASSES 8 and, for n > 1, packet
  shards (r, n, block 1); per iteration a zeroed ld of 8 planes takes the passes and the gather, then
  planes_r += ld.  Plane c comes from rank c % n, Ld is the planes added in class order.
* recipe B (partial films): the same with one plane, Ld = ((f_0 + f_1) + f_2) ...

Every context count dividing 8 must give recipe A's n = 1 image bit for bit; any other count recipe B's.
Against the single-context bre_render only the grouping of the float sums differs: relative L2 <= 1e-6 and
every pixel above 1e-3 of the maximum within 1e-4 (the bars tests/test_shard_gpu.py holds packet-shard
sums to)."""
import ctypes
import contextlib
import importlib
import os
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENES = os.path.join(ROOT, "scenes")

# 72 x 40: no multiple of the 16-pixel camera tiles or of 64 pixels; 2,880 primary segments are >= 45
# packets, so every one of the 8 packet classes occurs
W, H, PHOTONS, ITERS, DEPTH, R0, ALPHA = 72, 40, 20_000, 3, 5, 0.05, 0.5
OPT_STAGE_ALL = 122  # internal: stage every non-root source through the peer copy


@pytest.fixture(scope="module")
def scene(scene_mod_gpu):
    return scene_mod_gpu.cornell_scene(0.05, 0.5, 0.0)


def _params(sc, w=W, h=H, iters=ITERS, surfaces=True, photons=PHOTONS, end=None):
    return sc.render_params(w, h, iterations=iters, photons=photons, max_depth=DEPTH, radius=R0, alpha=ALPHA,
                            render_surfaces=surfaces, end_iteration=end)


@contextlib.contextmanager
def _contexts(bre, n, **kw):
    ctxs = [bre.BeamGather(0, **kw) for _ in range(n)]
    try:
        yield ctxs
    finally:
        for c in ctxs:
            c.close()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _same_bits(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _rel_l2(a, b):
    a, b = a.astype(np.float64), b.astype(np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def _within_sum_order(got, want):
    """The bars of tests/test_shard_gpu.py:89-91."""
    got, want = got.reshape(-1, 3), want.reshape(-1, 3)
    l2 = _rel_l2(got, want)
    big = want.max(axis=1) > 1e-3 * want.max()
    worst = float((np.abs(got - want)[big] / np.abs(want[big]).max(axis=1, keepdims=True)).max())
    print(f"rel L2 {l2:.3e}, worst big-pixel error {worst:.3e}")
    return l2 <= 1e-6 and worst <= 1e-4


def _recipe_film(bre, scene, p, rank, n, classes):
    """Rank `rank` of n's film after the iterations of p: float32 [classes, 3 * npix]."""
    import torch

    npix = p.width * p.height
    # one stream of torch's for the context and for the fills and adds below, so that they run in stream
    # order (the legacy default stream is not ordered against a context's own non-blocking stream, and its
    # handle 0 would select that one)
    stream = torch.cuda.Stream()
    assert stream.cuda_stream != 0
    with torch.cuda.stream(stream), bre.BeamGather(0) as g:
        film = torch.zeros((classes * npix, 3), dtype=torch.float32, device="cuda")
        g.set_stream(stream.cuda_stream)
        g.set_film_classes(classes)
        if n > 1:
            g.set_shard(rank, n, 1, packets=True)
        for it in range(p.start_iteration, p.end_iteration):
            R = bre.beam_radius_at(p.initial_radius, p.alpha, it)
            ld = torch.zeros_like(film)
            g.trace_photons(scene, p.photons_per_iteration, it, p.max_depth, R)
            g.camera_pass(scene, p.width, p.height, it, p.max_depth, bool(p.render_surfaces), True, surface=ld)
            g.gather_camera(R, ld)
            film += ld
        g.synchronize()
    torch.cuda.synchronize()
    return film.cpu().numpy().reshape(classes, 3 * npix)


def _resolve(bre, ld, p):
    out = np.zeros_like(ld)
    assert bre.load_library().bre_resolve_image(p.width * p.height, ld.ctypes.data, p.end_iteration - 1,
                                                out.ctypes.data) == 0
    return out.reshape(p.height, p.width, 3)


def _recipe_a(bre, scene, p, n):
    """(image, the 8 planes as gathered from the n ranks)."""
    films = [_recipe_film(bre, scene, p, r, n, 8) for r in range(n)]
    planes = np.stack([films[c % n][c] for c in range(8)])
    ld = planes[0].copy()
    for c in range(1, 8):
        ld = ld + planes[c]
    return _resolve(bre, ld, p), planes


def _recipe_b(bre, scene, p, n):
    films = [_recipe_film(bre, scene, p, r, n, 1)[0] for r in range(n)]
    ld = films[0].copy()
    for f in films[1:]:
        ld = ld + f
    return _resolve(bre, ld, p)


def _sharded(bre, scene, p, n, stage_all=False):
    with _contexts(bre, n) as ctxs:
        if stage_all:
            ctxs[0].set_option(OPT_STAGE_ALL, 1)
        return bre.render_sharded(ctxs, scene, p)


@pytest.fixture(scope="module")
def images(bre, scene, scene_mod_gpu):
    """bre_render_sharded's image per context count, rendered once and shared (never modified)."""
    cache = {}

    def get(n):
        if n not in cache:
            cache[n] = _sharded(bre, scene, _params(scene_mod_gpu), n)
            cache[n].setflags(write=False)
        return cache[n]

    return get


@pytest.mark.parametrize("surfaces", [True, False])
def test_bitwise_across_context_counts(bre, scene, scene_mod_gpu, images, surfaces):
    """1, 2, 4 and 8 contexts give recipe A's one-rank image bit for bit, with the surface radiance and
    with the planes holding gather terms only; the input exercises every class plane."""
    p = _params(scene_mod_gpu, surfaces=surfaces)
    want, planes = _recipe_a(bre, scene, p, 1)
    for c in range(8):
        assert planes[c].any(), f"class plane {c} is empty: the input no longer exercises every class"
    assert want.max() > 0
    for n in (1, 2, 4, 8):
        got = images(n) if surfaces else _sharded(bre, scene, p, n)
        assert _same_bits(got, want), n


def test_recipe_a_shards_give_the_one_rank_planes(bre, scene, scene_mod_gpu):
    """The recipe itself: the planes gathered from 4 ranks are the one-rank planes (what makes the
    sharded image independent of the count)."""
    p = _params(scene_mod_gpu)
    img1, planes1 = _recipe_a(bre, scene, p, 1)
    img4, planes4 = _recipe_a(bre, scene, p, 4)
    assert _same_bits(planes4, planes1) and _same_bits(img4, img1)


def test_three_contexts_sum_in_context_order(bre, scene, scene_mod_gpu, images):
    p = _params(scene_mod_gpu)
    got = images(3)
    assert _same_bits(got, _recipe_b(bre, scene, p, 3))
    assert _same_bits(_sharded(bre, scene, p, 3), got)  # the same bits from run to run
    assert _within_sum_order(got, images(1))


def test_one_context_against_bre_render(bre, scene, scene_mod_gpu, images):
    p = _params(scene_mod_gpu)
    with bre.BeamGather(0) as g:
        want = g.render(scene, p)
    assert _within_sum_order(images(1), want)


@pytest.mark.parametrize("n", [4, 3])
def test_staged_sources_give_the_same_bits(bre, scene, scene_mod_gpu, images, n):
    """Internal option 122 on context 0: every non-root source goes through the staging buffer and the
    peer copy (the cross-device path, on one GPU)."""
    got = _sharded(bre, scene, _params(scene_mod_gpu), n, stage_all=True)
    assert _same_bits(got, images(n))


@pytest.mark.parametrize("n", [1, 2, 3])
def test_film_with_unaligned_planes(bre, scene, scene_mod_gpu, n):
    """25 x 15: a plane holds 1,125 floats, so planes 1, 2, 3, 5 ... start off a 16-byte boundary and the
    collective takes its scalar path; two iterations."""
    p = _params(scene_mod_gpu, w=25, h=15, iters=2, photons=5000)
    got = _sharded(bre, scene, p, n)
    want = _recipe_b(bre, scene, p, 3) if n == 3 else _recipe_a(bre, scene, p, 1)[0]
    assert want.max() > 0
    assert _same_bits(got, want)
    assert _same_bits(_sharded(bre, scene, p, n, stage_all=True), want)


def test_progressive_schedule_and_stop(bre, scene, scene_mod_gpu):
    p = _params(scene_mod_gpu, iters=5)
    seen = []
    with _contexts(bre, 2) as ctxs:
        bre.render_progressive_sharded(ctxs, scene, p, 2, lambda it, img: seen.append((it, img)))
        # (iter + 1) % 2 == 0 -> iterations 1 and 3; iter + 1 == end -> 4
        assert [it for it, _ in seen] == [1, 3, 4]
        for it, img in seen:
            want = bre.render_sharded(ctxs, scene, _params(scene_mod_gpu, iters=5, end=it + 1))
            assert _same_bits(img, want), it
        # a callback that refuses stops the render with BRE_ERR_STATE; the contexts stay usable
        calls = []
        with pytest.raises(bre.BreError) as e:
            bre.render_progressive_sharded(ctxs, scene, p, 1, lambda it, img: calls.append(it) or 1)
        assert e.value.status == 4 and calls == [0]
        with bre.BeamGather(0) as g:
            want = g.render(scene, _params(scene_mod_gpu))
        for c in ctxs:
            assert _same_bits(c.render(scene, _params(scene_mod_gpu)), want)


def test_a_failing_context_stops_all_and_none_is_left_waiting(bre, scene, scene_mod_gpu, images):
    """A device error flag on context 1 (a traversal-stack overflow: internal option 101 with one work root,
    as tests/test_gpu_parity.py forces it) surfaces at that context's next synchronising call, in the
    middle of the render: every context stops at an iteration boundary, the call returns context 1's
    status and message, and both contexts render normally afterwards."""
    p = _params(scene_mod_gpu, iters=4)
    with _contexts(bre, 2) as ctxs:
        ctxs[1].set_option(bre.OPT_SPLIT, 1)
        ctxs[1].set_option(101, 2)  # a 2-entry traversal stack
        calls = []
        with pytest.raises(bre.BreError, match="context 1:.*stack overflow") as e:
            bre.render_progressive_sharded(ctxs, scene, p, 1, lambda it, img: calls.append(it))
        assert e.value.status == 4
        assert len(calls) < 4  # stopped before the end
        ctxs[1].set_option(101, 0)
        ctxs[1].set_option(bre.OPT_SPLIT, 256)
        assert _same_bits(bre.render_sharded(ctxs, scene, _params(scene_mod_gpu)), images(2))


def test_empty_range_and_null_callback(bre, scene, scene_mod_gpu):
    with _contexts(bre, 2) as ctxs:
        img = bre.render_sharded(ctxs, scene, _params(scene_mod_gpu, end=0))
        assert img.shape == (H, W, 3) and not img.any()
        bre.render_progressive_sharded(ctxs, scene, _params(scene_mod_gpu, iters=2), 1, None)


def test_options_are_restored(bre, scene, scene_mod_gpu, images):
    import torch

    p = _params(scene_mod_gpu)
    with bre.BeamGather(0) as g:
        want = g.render(scene, p)

    def one_iteration(g):
        ld = torch.zeros((8 * W * H, 3), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()  # the fill, before the context's own stream writes the film
        g.render_iteration(scene, p, 1, ld)
        g.synchronize()
        return ld.cpu().numpy()

    with _contexts(bre, 2) as ctxs:
        assert _same_bits(bre.render_sharded(ctxs, scene, p), images(2))
        assert _same_bits(ctxs[1].render(scene, p), want)  # bre_render refuses film classes: none are left set
        # shard options and film classes of the caller's own survive the call
        ctxs[1].set_film_classes(8)
        ctxs[1].set_shard(1, 2, 1, packets=True)
        assert _same_bits(bre.render_sharded(ctxs, scene, p), images(2))
        got = one_iteration(ctxs[1])
    with bre.BeamGather(0) as g:
        g.set_film_classes(8)
        g.set_shard(1, 2, 1, packets=True)
        fresh = one_iteration(g)
    planes = fresh.reshape(8, -1)
    assert planes[1].any() and not planes[0].any()  # rank 1 of 2 owns the odd planes
    assert _same_bits(got, fresh)


def test_refusals_launch_nothing_and_leave_the_contexts_usable(bre, scene, scene_mod_gpu, images):
    lib = bre.load_library()
    p = _params(scene_mod_gpu)
    img = np.zeros((H, W, 3), np.float32)
    S, P = ctypes.addressof(scene), ctypes.addressof(p)

    def raw(ctxs, n, s=S, image=img):
        arr = (ctypes.c_void_p * len(ctxs))(*[c.h.value for c in ctxs])
        return lib.bre_render_sharded(arr, n, s, P, None if image is None else image.ctypes.data)

    with _contexts(bre, 9) as ctxs:
        two = ctxs[:2]
        # class-plane films need the deterministic compose of kernels 0 / 4
        ctxs[1].set_option(bre.OPT_KERNEL, 2)
        assert raw(two, 2) == 4
        assert lib.bre_last_error(ctxs[0].h).decode().startswith("context 1:")
        with pytest.raises(bre.BreError, match="context 1:"):
            bre.render_progressive_sharded(two, scene, p, 1, lambda it, im: 0)
        assert ctxs[1].stats()["n_photons"] == 0  # nothing ran
        ctxs[1].set_option(bre.OPT_KERNEL, 0)
        assert raw([ctxs[0], ctxs[0]], 2) == 1  # a repeated context
        assert "repeated" in lib.bre_last_error(ctxs[0].h).decode()
        assert raw(ctxs, 0) == 1
        assert raw(ctxs, 9) == 1
        assert raw(two, 2, image=None) == 1
        assert raw(two, 2, s=None) == 1
        assert not img.any()
        assert all(c.stats()["n_photons"] == 0 for c in ctxs)
        assert _same_bits(bre.render_sharded(two, scene, p), images(2))


@pytest.mark.parametrize("nctx", [2, 3, 4])
def test_gather_sharded_film_is_the_host_sum_bit_for_bit(bre, synth, nctx):
    """bre_gather_sharded's accum against the float32 restatement of the host sum it replaced: the
    contexts' partial films from per-context bre_gather calls with the shard options set by hand, added in
    context order, then added to the caller's film."""
    w = h = 16
    beams = synth.fog_beams(300, seed=4242, radius=0.05)
    a, b = synth.camera_segments(w, h, seed=99), synth.bounce_segments(244, seed=100, npix=w * h)
    segs = {k: np.concatenate([a[k], b[k]]) for k in a}
    assert segs["tmax"].shape[0] == 500
    R, npix = 0.05, w * h
    start = np.random.default_rng(7).random((npix, 3), dtype=np.float32)
    with _contexts(bre, nctx) as ctxs:
        parts = []
        for i, c in enumerate(ctxs):
            c.set_beams(beams["start"], beams["end"], beams["radius"], beams["power"])
            c.set_shard(i, nctx, 1, packets=True)
            film = np.zeros((npix, 3), np.float32)
            c.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], segs["pixel"], R=R, npix=npix, accum=film,
                     seg_rgb=False)
            c.set_shard(0, 1, 1)
            parts.append(film)
        v = parts[0].copy()
        for f in parts[1:]:
            v += f
        want = start + v
        assert v.any() and sum(f.any() for f in parts) == nctx
        got = start.copy()
        bre.gather_sharded(ctxs, segs["o"], segs["p"], segs["d"], segs["tmax"], segs["pixel"], R=R, npix=npix,
                           accum=got, seg_rgb=False)
    assert _same_bits(got, want)


def _small_scene_text():
    """The scene of tests/test_pbrt_gpu.py's SMALL: scenes/cornell_fog_c1.pbrt at 48 x 40, 3 iterations of
    20,000 photons, initial radius 0.05, the world file inlined."""
    text = open(os.path.join(SCENES, "cornell_fog_c1.pbrt")).read()
    text = (text.replace("[256]", "[48]", 1).replace("[256]", "[40]", 1)
            .replace('"integer iterations" [1]', '"integer iterations" [3]')
            .replace("[50000]", "[20000]")
            .replace('"float initialbeamradius" [0.01]', '"float initialbeamradius" [0.05]')
            .replace('Include "cornell_world.pbrt"', open(os.path.join(SCENES, "cornell_world.pbrt")).read()))
    return text


def test_mirror_and_command_line(tmp_path):
    pb = importlib.import_module("beam-radiance-estimate-pbrt_amd.pbrt")
    text = _small_scene_text()
    path = tmp_path / "small.pbrt"
    path.write_text(text)
    env = {k: v for k, v in os.environ.items() if k != "BRE_DEVICES"}

    def cli(name, *args, env=env):
        out = tmp_path / name
        r = subprocess.run([pb.CLI_PATH, *args, "--outfile", str(out), str(path)], capture_output=True, text=True,
                           timeout=120, env=env)
        assert r.returncode == 0, r.stderr
        return out.read_bytes(), pb.read_pfm(str(out))

    s = pb.parse_string(text)
    assert s.ok, s.messages
    assert (s.film["xres"], s.film["yres"], s.params.end_iteration) == (48, 40, 3)
    lib_out = tmp_path / "lib.pfm"
    s.render(device=0, outfile=str(lib_out), write_files=True)
    plain_bytes, plain = cli("plain.pfm")
    assert plain_bytes == lib_out.read_bytes()  # no flag, no BRE_DEVICES: exactly the one-context render
    two_bytes, two = cli("two.pfm", "--devices", "0,0")
    four_bytes, _ = cli("four.pfm", "--devices", "0,0,0,0")
    assert two_bytes == four_bytes
    assert plain.max() > 0 and _within_sum_order(two, plain)
    assert _same_bits(s.render(devices=[0, 0], write_files=False), two)
    # BRE_DEVICES naming more than one device selects them; one device does not
    env_bytes, _ = cli("env.pfm", env=dict(env, BRE_DEVICES="0,0"))
    assert env_bytes == two_bytes
    one_bytes, _ = cli("one.pfm", env=dict(env, BRE_DEVICES="0"))
    assert one_bytes == plain_bytes
