"""Shared pieces of tests/test_context_reuse_gpu.py: the named beam sets of its walks, one step of a walk
through the host or the device entry points, and the comparisons every step ends with (a long-lived
context against a fresh one bit for bit, and against the oracle at the bar of tests/test_gpu_parity.py)."""
import numpy as np
import pytest

from test_gpu_parity import SEG_RTOL, _seg_close  # the parity bar, not restated
from test_lbvh_gpu import _beam_set

STAT_KEYS = ("n_beams", "n_beams_valid", "n_nodes", "n_segments")
BRE_ERR_INVALID_ARG, BRE_ERR_STATE = 1, 4
SEG_KEYS = ("o", "p", "d", "tmax", "pixel")
BEAM_KEYS = ("start", "end", "radius", "power")


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype.itemsize == 4 else a


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


# ---- options of a live context, replayed on the fresh one ----
def set_opt(g, opts, key, value):
    """Set an option on g and record it (last set, last replayed: a shard count before its rank)."""
    g.set_option(key, value)
    opts.pop(key, None)
    opts[key] = value


def open_ctx(bre, opts):
    g = bre.BeamGather(0)
    for k, v in opts.items():
        g.set_option(k, v)
    return g


# ---- inputs ----
def beams_of(synth, name):
    """fog-N: synth.fog_beams(N, seed=100 + N), the sets under 100 beams with mean_length 0.6 so that a few
    segments still meet them; the other names as the walks' docstrings give them."""
    if name == "empty":
        return {"start": np.zeros((0, 3), np.float32), "end": np.zeros((0, 3), np.float32),
                "radius": np.zeros(0, np.float32), "power": np.zeros((0, 3), np.float32)}
    if name == "third-invalid-999":
        return _beam_set(synth, name)
    if name == "degenerate-50":
        b = synth.fog_beams(50, seed=150)
        b["end"] = b["start"].copy()  # every WorldBound is NaN: no valid beam
        return b
    if name == "fog-3000-radii":
        b = synth.fog_beams(3000, seed=3100)
        rng = np.random.default_rng(32)  # tests/test_radius_layout_gpu.py, the "random" kind
        b["radius"] = rng.uniform(0.004, 0.03, b["radius"].shape[0]).astype(np.float32)
        return b
    n = int(name[4:])
    if n < 100:
        return synth.fog_beams(n, seed=100 + n, mean_length=0.6)
    return synth.fog_beams(n, seed=100 + n)


def empty_segments():
    return {"o": np.zeros((0, 3), np.float32), "p": np.zeros((0, 3), np.float32), "d": np.zeros((0, 3), np.float32),
            "tmax": np.zeros(0, np.float32), "pixel": np.zeros(0, np.int32)}


def has_valid_beam(beams):
    return bool((beams["start"] != beams["end"]).any())  # a zero-length beam has a NaN WorldBound


def oracle_ref(oracle, beams, segs, R, sqrt_mode=0):
    """cand / contrib / seg_rgb of the reference: the SAH tree's gather, the brute force for a set with
    invalid beams (as test_zero_length_beams_never_gathered), zeros where there is nothing to gather."""
    nb, ns = beams["radius"].shape[0], segs["tmax"].shape[0]
    if nb == 0 or ns == 0 or not has_valid_beam(beams):
        return {"seg_rgb": np.zeros((ns, 3), np.float32), "cand": np.zeros(ns, np.int64),
                "contrib": np.zeros(ns, np.int64)}
    if (beams["start"] == beams["end"]).all(axis=1).any():
        ref = oracle.bruteforce(beams, segs, R, sqrt_mode=sqrt_mode, nthreads=8)
    else:
        ref = oracle.build(beams, sqrt_mode=sqrt_mode).gather(segs, R)
    assert int(ref["contrib"].sum()) > 0, "the step's inputs must contribute in the oracle alone"
    return ref


def film_base(npix):
    """A film that is not all zero (and has zeros), the same before every step."""
    return ((np.arange(3 * npix) % 7).astype(np.float32) * np.float32(0.125)).reshape(npix, 3)


def compose(film, pixel, seg_rgb):
    """The documented compose, sequentially in float32 (gather_segments' comment in bre_api_gather.hip, bre_sort.hip
    above k_pix_keys): per pixel s = 0, the pixel's seg_rgb rows added in the caller's order, then
    film[p] += s where s is not zero."""
    out = np.array(film, np.float32, copy=True)
    pixel = np.asarray(pixel, np.int64)
    n = pixel.shape[0]
    if n == 0:
        return out
    s = np.zeros_like(out)
    order = np.argsort(pixel, kind="stable")
    sp = pixel[order]
    start = np.r_[0, np.nonzero(np.diff(sp))[0] + 1]
    rank = np.arange(n) - np.repeat(start, np.diff(np.r_[start, n]))  # position within the pixel's run
    for r in range(int(rank.max()) + 1):
        idx = order[rank == r]  # at most one segment per pixel
        s[pixel[idx]] = s[pixel[idx]] + seg_rgb[idx]
    hit = (s != 0).any(axis=1)
    out[hit] = out[hit] + s[hit]
    return out


# ---- one step ----
def set_beams(g, beams, device=False):
    if device:
        import torch

        d = [torch.from_numpy(np.ascontiguousarray(beams[k], np.float32)).cuda().contiguous() for k in BEAM_KEYS]
        torch.cuda.synchronize()
        g.set_beams_device(*d)
    else:
        g.set_beams(*(beams[k] for k in BEAM_KEYS))


def check_get_beams(bre, g, beams, device):
    """After set_beams the set reads back as given; after set_beams_device with beams the library has no
    copy and says so (an empty device set reads back as the empty set): never the previous set."""
    if device and beams["radius"].shape[0] > 0:
        with pytest.raises(bre.BreError) as e:
            g.get_beams()
        assert e.value.status == BRE_ERR_STATE
        return
    got = g.get_beams()
    for k in BEAM_KEYS:
        assert same_bits(got[k], np.ascontiguousarray(beams[k], np.float32)), k


def gather(g, segs, R, npix=0, film=None, device=False, counts=True, pixel=True):
    """One gather through bre_gather (host arrays) or bre_gather_device (torch tensors, then synchronize):
    seg_rgb, counts, the film after it (a copy of `film` is added to) and the stats."""
    n = segs["tmax"].shape[0]
    pix = segs["pixel"] if pixel else None
    if not device:
        acc = None if film is None else np.array(film, np.float32, copy=True)
        out = g.gather(segs["o"], segs["p"], segs["d"], segs["tmax"], pix, R=R, npix=npix, accum=acc, counts=counts)
        out["accum"] = acc
    else:
        import torch

        d = {k: torch.from_numpy(np.ascontiguousarray(segs[k])).cuda().contiguous() for k in SEG_KEYS}
        rgb = torch.full((n, 3), float("nan"), dtype=torch.float32, device="cuda")
        cnt = torch.full((n, 2), -7, dtype=torch.int32, device="cuda") if counts else None
        acc = None if film is None else torch.from_numpy(np.array(film, np.float32, copy=True)).cuda()
        torch.cuda.synchronize()  # the fills above run on torch's stream, the gather on the context's
        g.gather_device(d["o"], d["p"], d["d"], d["tmax"], d["pixel"] if pixel else None, R, npix, accum=acc,
                        seg_rgb=rgb, counts=cnt)
        g.synchronize()
        out = {"seg_rgb": rgb.cpu().numpy(), "accum": None if acc is None else acc.cpu().numpy()}
        if counts:
            out["counts"] = cnt.cpu().numpy()
    out["stats"] = g.stats()
    return out


# ---- comparisons ----
def assert_same(got, want, what, film=True, counters=True):
    """The long-lived context's step against the fresh context's: outputs bit for bit, stats equal."""
    assert same_bits(got["seg_rgb"], want["seg_rgb"]), f"{what}: seg_rgb differs from a fresh context's"
    if "counts" in want:
        assert np.array_equal(got["counts"], want["counts"]), f"{what}: counts differ from a fresh context's"
    if film and want.get("accum") is not None:
        assert same_bits(got["accum"], want["accum"]), f"{what}: the film differs from a fresh context's"
    for k in STAT_KEYS + (("candidates", "contributions") if counters else ()):
        assert got["stats"][k] == want["stats"][k], (what, k, got["stats"][k], want["stats"][k])


def assert_oracle(got, ref, what, counters=True, cand=True):
    """The parity bar: exact counts, per-segment sums within SEG_RTOL of the segment's magnitude."""
    if "counts" in got:
        if counters and cand:
            assert np.array_equal(got["counts"][:, 0], ref["cand"]), f"{what}: candidate counts differ from the oracle's"
        elif not counters:
            assert (got["counts"][:, 0] == -1).all(), f"{what}: candidates are not counted with counters off"
        assert np.array_equal(got["counts"][:, 1], ref["contrib"]), f"{what}: contribution counts differ"
    if ref["seg_rgb"].shape[0]:
        err = _seg_close(got["seg_rgb"], ref["seg_rgb"])
        assert err <= SEG_RTOL, f"{what}: per-segment relative error {err}"
    if counters:
        if cand:
            assert got["stats"]["candidates"] == int(ref["cand"].sum()), what
        assert got["stats"]["contributions"] == int(ref["contrib"].sum()), what


def assert_film_composed(got, film0, segs, what):
    assert same_bits(got["accum"], compose(film0, segs["pixel"], got["seg_rgb"])), \
        f"{what}: the film is not the sequential compose of seg_rgb"
