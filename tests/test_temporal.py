"""crt_temporal: temporal accumulation by reprojection, held BY BYTES to tests/temporal_ref.py, the definition in float32
numpy.  The reference's inputs are the handle's own read_sum() / read_denoised() and read_aov(), which other tests hold to the oracle, and
the oracle's primary-ray directions of the recorded view, so each check isolates the reprojection and the blend.

CPU: the ABI and the Python surface (T0), the premises the GPU checks rest on (T1: every way a pixel or a tap can lose its history
occurs), properties of the definition (T2) and its quality (T3).  GPU: flat scenes over a moving camera (G1), an instanced scene across
refits and a set (G2), the denoised source (G3), nothing else moves (G4), refusals and ordering (G5), memory (G6)."""
import ctypes as C
import inspect
import os
import re
import types

import numpy as np
import pytest

from denoise_ref import filterable, prepare
from temporal_ref import CENSUS, temporal_ref, view_record
from test_aov import CHANNELS, bit_of, device_bytes_at, flat_data, flat_reference, flat_scene, frames_state, identity_scene, instanced_reference, read_all, words
from test_denoise import SIZES as DENOISE_SIZES, SMALL, camera_w, device_bytes_in_use, guides, two_walls
from test_instances_frames import RVS, flat_variants, primary_oracle, shading_of
from test_instances_oracle import host_blas, host_scene, is_identity, orc

f32 = np.float32
SIZES = (DENOISE_SIZES[0], SMALL)                            # 67 x 45: partial 16 x 16 blocks both ways; 20 x 9: shorter than one block
NAMES = ["cornell", "textured", "tess8_mat"]
ENTRIES = ("crt_temporal", "crt_temporal_reset", "crt_read_temporal", "crt_read_temporal_history", "crt_temporal_device", "crt_resolve_temporal",
           "crt_resolve_temporal_device")
GUIDES = ("HIT", "IDS", "NORMAL", "ALBEDO")


def moved_camera(cam, right=0.0, up=0.0, forward=0.0):
    """a copy of `cam` translated along its own basis (float32 adds); the basis and the field of view stay"""
    from caitlynrenderer_amd._lib import crt_camera
    c = crt_camera()
    C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(c))
    pos = np.array(cam.c.position[:], f32)
    for amount, axis in ((right, cam.c.right), (up, cam.c.up), (forward, cam.c.forward)):
        pos = (pos + (f32(amount) * np.array(axis[:], f32)).astype(f32)).astype(f32)
    for k in range(3):
        c.position[k] = float(pos[k])
    return types.SimpleNamespace(c=c)


def directions(ob, cam, W, H, rv, jitter=True):
    return primary_oracle(ob, cam, W, H).primary_rays(rv[0], rv[1], jitter=bool(jitter))["d"].reshape(H, W, 3)


def params_of(flags=1, max_history=32, sigma_depth=0.1, normal_min=0.9):
    return dict(demodulate=bool(flags & 1), clamp=bool(flags & 2), max_history=max_history, sigma_depth=sigma_depth, normal_min=normal_min)


# ---------------------------------------------------------------- T0 ----

def test_t0_header_exports_and_binding_agree(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS and hasattr(raw, name) and hasattr(L, name), name
    assert re.search(r"CRT_TEMPORAL_DEMODULATE = 1, CRT_TEMPORAL_CLAMP = 2\b", code)
    assert re.search(r"CRT_TEMPORAL_SOURCE_SUM = 0, CRT_TEMPORAL_SOURCE_DENOISED = 1\b", code)
    assert (_lib.CRT_TEMPORAL_DEMODULATE, _lib.CRT_TEMPORAL_CLAMP, _lib.CRT_TEMPORAL_SOURCE_SUM, _lib.CRT_TEMPORAL_SOURCE_DENOISED) == (1, 2, 0, 1)
    P = _lib.crt_temporal_params
    assert C.sizeof(P) == 32
    fields = re.search(r"typedef struct crt_temporal_params \{(.*?)\} crt_temporal_params;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", fields) == [n for n, _ in P._fields_]
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("flags", 0), ("source", 4), ("max_history", 8), ("sigma_depth", 12), ("normal_min", 16), ("reserved", 20)]
    assert L.crt_abi_version() == 6
    for name in ("temporal", "temporal_reset", "read_temporal", "read_temporal_history", "temporal_device", "resolve_temporal", "resolve_temporal_device"):
        assert callable(getattr(cr.Scene, name))
    sig = inspect.signature(cr.Scene.temporal)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("inv_count", None), ("source", "sum"), ("demodulate", True), ("clamp", False), ("max_history", 32),
                                                                          ("sigma_depth", 0.1), ("normal_min", 0.9), ("sync", True)]
    # a null scene is refused before anything else, with a reason, and without a GPU
    buf = np.zeros(16, np.uint8)
    p = C.c_void_p()
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.crt_temporal(None, 1.0, None, 1) == _lib.CRT_ERR_INVALID and b"null" in L.crt_last_error()
    assert L.crt_temporal_reset(None) == _lib.CRT_ERR_INVALID
    assert L.crt_read_temporal(None, ptr, 4) == _lib.CRT_ERR_INVALID
    assert L.crt_read_temporal_history(None, ptr, 4) == _lib.CRT_ERR_INVALID
    assert L.crt_temporal_device(None, C.byref(p)) == _lib.CRT_ERR_INVALID and not p.value
    assert L.crt_resolve_temporal(None, ptr, 16) == _lib.CRT_ERR_INVALID
    assert L.crt_resolve_temporal_device(None, C.byref(p), 1) == _lib.CRT_ERR_INVALID and not p.value
    assert not buf.any()


# ---------------------------------------------------------------- T1 - T3: on the oracle ----

_VIEWS = {}


def oracle_view(cr, ob, cornell, tag, cam, W, H, rv, jitter=True, depth=3):
    """(one oracle frame of the Cornell box from `cam`, its guides, its primary directions, the view record), computed once per tag"""
    key = (tag, W, H, rv, jitter, depth)
    if key not in _VIEWS:
        mesh, _ = cornell
        data = flat_data(cr, mesh, cornell[1], "sbvh")
        o = ob.Oracle(data, W, H, depth, camera=cam)
        assert jitter                                           # the oracle's frames are jittered
        frame, _ = o.render_frame(rv[0], rv[1], threads=16)
        aov = guides(flat_reference(cr, ob, "cornell/" + tag, "sbvh", mesh, data, cam, W, H, rv, 1))
        _VIEWS[key] = (frame, aov, directions(ob, cam, W, H, rv), view_record(cam, W, H))
    return _VIEWS[key]


def run(seq, params):
    """the reference over a sequence of (source, aov, d, view[, o2w, w2o]); returns the last call's (image, N, state, census)"""
    state, out = None, None
    for item in seq:
        out = temporal_ref(state, item[0], item[1], item[2], item[3], *(item[4:6] if len(item) > 4 else (None, None)), params)
        state = out[2]
    return out


def walls_view(cr, ob, w, M, mesh_of, offs, W, H, rv):
    """the two-walls scene of test_denoise with the transforms M: (guides, directions, view, o2w, w2o) from the two-level oracle"""
    cam = camera_w(cr)
    s = host_scene(cr, [host_blas(cr, m) for m in w["meshes"]], list(M), list(mesh_of))
    rays = primary_oracle(ob, cam, W, H).primary_rays(*rv, jitter=True)
    hits, ids, _, _, refused = orc(ob, s, rays)
    assert refused.sum() == 0
    w2o = np.array([cr.instance_inverse(m) for m in M], f32).reshape(-1, 3, 4)
    ident = np.array([is_identity(m) for m in M])
    ref = instanced_reference(cr, W, H, rays, hits, ids, w["meshes"], mesh_of, offs, w["table"], None, w2o, ident)
    return guides(ref), rays["d"].reshape(H, W, 3), view_record(cam, W, H), np.asarray(M, f32).reshape(-1, 3, 4), w2o


def pan_step(aov, view, W, pixels):
    """the sideways camera move that shifts a surface at the view's median depth by `pixels` pixels"""
    t = aov["HIT"]["t"][aov["HIT"]["tri"] >= 0]
    return float(pixels * 2.0 * np.median(t) * view["aspect_tan"] / W)


def test_t1_every_way_of_losing_history_occurs(cr, ob, cornell):
    """Measured here at 67 x 45 (3,015 pixels; Cornell: 2,008 F), the second call's census:
    static view, jitter: 1,982 with history, 18 below the weight; taps: 7,132 counted, 54 edge, 154 key (on a flat scene: a neighbour that
    is not F), 568 normal, 92 depth.
    pan of 3 pixels: 1,974 with history, 21 without (all below the weight: the box does not reach the frame's sides, so no pixel leaves
    the frame on a pan); taps 54 edge, 155 key, 592 normal, 82 depth.
    previous camera inside the box: 76 behind it, 1,508 off its frame, 74 below the weight, 350 with history.
    two walls, wall 1 translated: 1,168 F, 588 pixels on the matrix path (wall 1) and 580 not, 184 taps cut by the key, 1 pixel below the weight.
    two walls after a third instance arrived: 1,365 F, 767 pixels of a new instance.
    CLAMP on the pan: 1,974 with history, the clamp changed h in 293."""
    W, H = SIZES[0]
    cam = cornell[1]
    P = params_of(1)
    base = oracle_view(cr, ob, cornell, "base0", cam, W, H, RVS[0])
    again = oracle_view(cr, ob, cornell, "base1", cam, W, H, RVS[1])
    nF = int(filterable(base[1]).sum())
    # a static view with jitter
    _, N, _, cs = run([base, again], P)
    print("T1 static:", cs)
    assert cs["with_history"] > 0.9 * nF and cs["tap_counted"] > 0 and cs["behind"] == 0 == cs["new_instance"]
    # a sideways pan of a few pixels: the frame edge, depth and normal cuts, pixels without history
    step = pan_step(base[1], base[3], W, 3.0)
    pan = oracle_view(cr, ob, cornell, "pan", moved_camera(cam, right=step), W, H, RVS[1])
    _, N, _, cs_pan = run([base, pan], P)
    print("T1 pan:", cs_pan)
    for name in ("low_weight", "tap_edge", "tap_key", "tap_normal", "tap_depth", "with_history", "without_history"):
        assert cs_pan[name] > 0, (name, cs_pan)
    assert (N[filterable(pan[1])] == 1).sum() == cs_pan["without_history"]
    # the previous camera inside the box, ahead of the current one: points behind it
    ahead = float(0.75 * np.median(base[1]["HIT"]["t"][base[1]["HIT"]["tri"] >= 0]))
    inside = oracle_view(cr, ob, cornell, "inside", moved_camera(cam, forward=ahead), W, H, RVS[1])
    _, _, _, cs = run([inside, base], P)
    print("T1 previous camera inside:", cs)
    assert cs["behind"] > 0 and cs["off_frame"] > 0 and cs["with_history"] > 0     # the box's border lies outside the closer camera's frame
    # two walls, one translated between the calls: key cuts, the matrix path for one instance and not for the other
    w = two_walls(cr)
    rng = np.random.default_rng(5)
    src = [rng.uniform(0.1, 2.0, (H, W, 3)).astype(f32) for _ in range(3)]
    M2 = w["M"].copy()
    M2[1, :, 3] += np.array([0.3, 0.2, 0.0], f32)
    v0 = walls_view(cr, ob, w, w["M"], w["mesh_of"], w["offs"], W, H, RVS[0])
    v1 = walls_view(cr, ob, w, M2, w["mesh_of"], w["offs"], W, H, RVS[1])
    _, _, _, cs = run([(src[0],) + v0, (src[1],) + v1], P)
    print("T1 two walls, one moved:", cs)
    in_view = v1[0]["IDS"]["instance"][filterable(v1[0])]
    assert cs["tap_key"] > 0 and cs["moved"] == (in_view == 1).sum() > 0 and (in_view == 0).sum() > 0
    # ... and after the instance count grew: pixels of an instance the previous call did not have
    M3 = np.concatenate([M2, np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5]]], f32)])
    v2 = walls_view(cr, ob, w, M3, np.array([0, 0, 0]), np.array([0, 1, 0], np.uint32), W, H, RVS[2])
    _, _, _, cs = run([(src[0],) + v0, (src[1],) + v1, (src[2],) + v2], P)
    print("T1 two walls, a third instance:", cs)
    assert cs["new_instance"] == (v2[0]["IDS"]["instance"][filterable(v2[0])] == 2).sum() > 0
    # CLAMP on the pan
    _, _, _, cs = run([base, pan], params_of(3))
    print("T1 clamp on the pan:", cs)
    assert cs["clamped"] > 0 and cs["with_history"] == cs_pan["with_history"]
    assert set(CENSUS) >= set(cs)


def static_inputs(cr, ob, cornell, W, H, k):
    """k one-frame sources of ONE static view without jitter in the guides (the frames themselves are the oracle's, jittered)"""
    mesh, cam = cornell
    data = flat_data(cr, mesh, cam, "sbvh")
    aov = guides(flat_reference(cr, ob, "cornell/static", "sbvh", mesh, data, cam, W, H, RVS[0], 0))
    d = directions(ob, cam, W, H, RVS[0], jitter=False)
    o = ob.Oracle(data, W, H, 3, camera=cam)
    return [o.render_frame(rv[0], rv[1], threads=16)[0] for rv in RVS[:k]], aov, d, view_record(cam, W, H)


def test_t2_properties_of_the_definition(cr, ob, cornell):
    """Static view, jitter 0.  N is held to min(k, max_history) within 8 * k ulp: the gathered length is a quotient of two sums of at
    most four products (about 6 roundings), and that error is carried through k calls (measured: 0).
    "The output equals the source to 1e-5 relative" is held relative to the frame's largest source value, not to each pixel's own: the
    reprojected position of a static pixel is its own centre only to about W * 2^-23 * a few = 1e-5 pixels, so the definition gathers
    the neighbour with a weight of that size, and a one-sample frame has pixels that are exactly 0 beside pixels that are not.  Measured
    here over 5 calls: error / peak 4e-8, 1.8e-6, 3.7e-6, 4.9e-6, 5.7e-6 (per pixel against its own value: up to 3.4e-4, and 266 .. 396
    pixels whose source is 0 and whose output is not)."""
    W, H = SIZES[0]
    frames, aov, d, view = static_inputs(cr, ob, cornell, W, H, 6)
    F = filterable(aov)
    assert 0 < F.sum() < F.size
    # the same source k times
    P = params_of(1, max_history=3)
    state = None
    for k in range(1, 6):
        image, N, state, cs = temporal_ref(state, frames[0], aov, d, view, None, None, P)
        want = min(k, 3)
        assert np.abs(N[F] - want).max() <= 8 * k * want * 2.0 ** -23, (k, np.abs(N[F] - want).max())
        assert (N[~F] == 1).all()
        err = np.abs(image - frames[0]).max() / np.abs(frames[0]).max()
        print(f"T2 the same source, call {k}: N error {np.abs(N[F] - want).max():.3g}, largest |output - source| / the frame's peak {err:.3g}")
        assert err <= 1e-5, k
        assert cs["with_history"] == (F.sum() if k > 1 else 0)
    # different one-frame sources, max_history 4096: the running mean
    P = params_of(1, max_history=4096)
    state, total = None, np.zeros((H, W, 3), np.float64)
    for k, frame in enumerate(frames, 1):
        image, N, state, _ = temporal_ref(state, frame, aov, d, view, None, None, P)
        total += frame
        mean = total / k
        err = np.abs(image - mean)[F].max() / mean[F].max()     # relative to the frame's peak, for the reason above
        print(f"T2 running mean after {k}: largest error on F pixels / the mean's peak {err:.3g}")
        assert err <= 1e-4, k
    # max_history 1: x times the divisor, by bytes; and it is history-less however long the history
    c, x, m, _, _, _, _ = prepare(frames[1], aov, 1.0, True)
    image, N, state1, cs = temporal_ref(state, frames[1], aov, d, view, None, None, params_of(1, max_history=1))
    want = np.where(F[..., None], (x * m).astype(f32), c)
    assert np.array_equal(image.view(np.uint32), want.view(np.uint32)) and (N == 1).all() and cs["with_history"] == 0
    # after a reset (no state), and after a toggle of DEMODULATE: N is 1 everywhere
    for st, flags in ((None, 1), (state, 0)):
        _, N, _, cs = temporal_ref(st, frames[2], aov, d, view, None, None, params_of(flags))
        assert (N == 1).all() and cs["with_history"] == 0 and cs["without_history"] == F.sum()


def test_t3_the_definition_removes_noise(cr, ob, cornell):
    """Cornell at 96 x 64, max_depth 3, a static view with jitter, 8 one-frame calls, against test_denoise C3's 256-frame oracle mean.
    Measured here: MSE(temporal after 8 calls) / MSE(the 8th frame alone) = 0.249 (1 / 8 is the ideal; the bilinear resampling of the
    jittered history adds bias, and pixels at silhouettes restart).  Asserted at 1.5 x that, 0.374, which is below 0.5."""
    W, H = 96, 64
    mesh, cam = cornell
    data = flat_data(cr, mesh, cam, "sbvh")
    o = ob.Oracle(data, W, H, 3, camera=cam)
    rng = np.random.default_rng(2024)
    ref = np.zeros((H, W, 3), f32)
    for rx, ry in rng.uniform(0.0, 1.0, (256, 2)):
        o.render_frame(rx, ry, ref, threads=16)
    ref = ref.astype(np.float64) / 256.0
    state = None
    for k in range(8):
        frame, aov, d, view = oracle_view(cr, ob, cornell, f"t3/{k}", cam, W, H, RVS[k])
        image, N, state, cs = temporal_ref(state, frame, aov, d, view, None, None, params_of(1))
    assert np.isfinite(image).all()
    mse_one, mse_out = np.mean((frame - ref) ** 2), np.mean((image - ref) ** 2)
    print(f"T3: MSE one frame {mse_one:.5g}, temporal {mse_out:.5g}, ratio {mse_out / mse_one:.3f}; last census {cs}")
    assert mse_out <= 1.5 * 0.249 * mse_one and 1.5 * 0.249 < 0.5


# ---------------------------------------------------------------- GPU ----

def check_call(cr, ob, sc, state, d, view, o2w, w2o, what, flags=1, max_history=32, source="sum", inv=1.0, **kw):
    """one crt_temporal against the definition on the handle's own source and guides, by bytes: image, N, RGBA8 and both device
    pointers.  Returns the reference's new state"""
    W, H = sc.width, sc.height
    src = (sc.read_sum() * f32(inv)).astype(f32) if source == "sum" else sc.read_denoised()
    aov = {n: sc.read_aov(bit_of(cr, n)) for n in GUIDES}
    P = dict(params_of(flags, max_history), **kw)
    want, want_n, new_state, census = temporal_ref(state, src, aov, d, view, o2w, w2o, P)
    sc.temporal(inv, source=source, sync=True, **P)
    got, got_n = sc.read_temporal(), sc.read_temporal_history()
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(2) | (got_n.view(np.uint32) != want_n.view(np.uint32)))
    print(f"{what} flags {flags} max_history {max_history}: differing pixels {bad[0].size}; with history {census['with_history']}, without {census['without_history']}")
    assert bad[0].size == 0, (what, flags, max_history, bad[0].size, bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4], got_n[bad][:4], want_n[bad][:4])
    rgba = ob.resolve(want, 1.0)
    assert np.array_equal(sc.resolve_temporal(), rgba), what
    p, q = sc.temporal_device(), sc.resolve_temporal_device()
    assert p and np.array_equal(device_bytes_at(p, W * H * 12), np.ascontiguousarray(want).view(np.uint8).reshape(-1)), what
    assert q and np.array_equal(device_bytes_at(q, W * H * 4), np.ascontiguousarray(rgba).reshape(-1)), what
    return new_state, census


def camera_path(cam, aov_t, view, W):
    """static, pan, dolly, pan back"""
    step = float(2.5 * 2.0 * aov_t * view["aspect_tan"] / W)
    return [cam, moved_camera(cam, right=step), moved_camera(cam, right=step, forward=0.08 * aov_t), moved_camera(cam, forward=0.08 * aov_t)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_g1_flat_scenes_over_a_moving_camera_by_bytes(cr, ob, cornell, textured, name):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    for W, H in SIZES:
        sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
        sc.set_option("jitter", 1)
        sc.render_aov(*RVS[0])
        hit = sc.read_aov(cr.AOV_HIT)
        cams = camera_path(cam, float(np.median(hit["t"][hit["tri"] >= 0])), view_record(cam, W, H), W)
        moved_on = 0
        for flags in (0, 1, 2, 3):
            for max_history in (2, 32):
                for form in ((1, 2) if flags & 2 else (0,)):
                    sc.set_option("temporal_form", form)
                    sc.temporal_reset()
                    state = None
                    for k, c in enumerate(cams):
                        sc.update(c)
                        sc.reset()
                        sc.render_frame(*RVS[k])
                        sc.render_aov(*RVS[k])
                        state, cs = check_call(cr, ob, sc, state, directions(ob, c, W, H, RVS[k]), view_record(c, W, H), None, None,
                                               f"G1 {name} {W}x{H} form {form} call {k}", flags, max_history)
                        assert (cs["with_history"] > 0) == (k > 0)
                        moved_on += cs["without_history"] if k else 0
        assert moved_on > 0                                   # the moves did cost some pixels their history
        sc.close()


def walls_handle(cr, W, H, capacity=4, depth=3):
    w = two_walls(cr)
    inst = cr.InstancedScene(w["meshes"], cr.instances_array(w["M"], w["mesh_of"], material_offsets=w["offs"]), capacity=capacity)
    sc = inst.frame_scene(shading_of(w["meshes"]), w["table"], w["light"], W, H, depth)
    sc.update(camera_w(cr))
    return w, inst, sc


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [1, 3])
def test_g2_an_instanced_scene_across_two_refits_and_a_set(cr, ob, flags):
    W, H = SIZES[0]
    w, inst, sc = walls_handle(cr, W, H)
    cam = camera_w(cr)
    view = view_record(cam, W, H)
    M1 = w["M"].copy()
    M1[1, :, 3] += np.array([0.3, 0.2, 0.0], f32)
    M2 = M1.copy()
    M2[1, :, 3] += np.array([-0.15, 0.1, 0.25], f32)
    M3 = np.concatenate([M2, np.array([[[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0.5]]], f32)])
    steps = [("created", None, w["M"]), ("refit", "refit", M1), ("refit again", "refit", M2), ("set", "set", M3)]
    state, seen = None, {}
    for k, (what, how, M) in enumerate(steps):
        n = M.shape[0]
        arr = cr.instances_array(M, np.zeros(n, np.int64), material_offsets=np.array([0, 1, 0][:n], np.uint32))
        if how:
            getattr(inst, how)(arr)
        sc.reset()
        sc.render_frame(*RVS[k])
        sc.render_aov(*RVS[k])
        o2w, w2o = inst.object_to_world().reshape(-1, 3, 4), inst.world_to_object().reshape(-1, 3, 4)
        assert np.array_equal(o2w.view(np.uint32), np.asarray(M, f32).view(np.uint32))
        state, cs = check_call(cr, ob, sc, state, directions(ob, cam, W, H, RVS[k]), view, o2w, w2o, f"G2 {what}", flags, 32)
        seen[what] = cs
    assert seen["refit"]["moved"] > 0 and seen["refit"]["tap_key"] > 0 and seen["refit"]["with_history"] > seen["refit"]["moved"]
    assert seen["refit again"]["moved"] > 0 and seen["set"]["new_instance"] > 0 and seen["set"]["moved"] == 0
    sc.close()
    inst.close()


@pytest.mark.gpu
def test_g3_the_denoised_source(cr, ob, cornell, textured):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[0]
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:2])
    sc.render_aov(*RVS[0])
    with pytest.raises(CrtError) as e:
        sc.temporal(0.5, source="denoised")
    assert e.value.code == CRT_ERR_INVALID
    state = None
    for k in range(3):
        sc.reset()
        sc.render_frames(RVS[k:k + 2])
        sc.render_aov(*RVS[k])
        sc.denoise(0.5, passes=3)
        denoised = sc.read_denoised()
        # inv_count is checked but not used: 0.125 here, against a reference that is given the denoised image as it is
        state, _ = check_call(cr, ob, sc, state, directions(ob, cam, W, H, RVS[k]), view_record(cam, W, H), None, None, f"G3 call {k}", 3, 32,
                              source="denoised", inv=0.125)
        assert np.array_equal(sc.read_denoised().view(np.uint32), denoised.view(np.uint32))
    assert (sc.read_temporal().view(np.uint32) != denoised.view(np.uint32)).any()
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g4_it_disturbs_nothing(cr, ob, cornell, textured, kind):
    """3 frames, render_aov, denoise, two temporal calls, 2 frames: sum, count and stats of 5 frames alone (test_aov G7's rule for the
    queue-order counts); every AOV channel, the denoised image and crt_resolve_device's buffer keep their bytes; crt_reset keeps N"""
    mesh, parts = flat_variants(cr, cornell, textured)["tess8_mat"]
    cam = cornell[1]
    W, H = SIZES[0]
    depth = 3

    def make():
        if kind == "flat":
            sc = flat_scene(cr, mesh, cam, "sbvh", W, H, depth)
            closer = sc.close
        else:
            inst, sc, _ = identity_scene(cr, mesh, parts, "sah", W, H, depth)
            sc.update(cam)
            closer = lambda: (sc.close(), inst.close())
        sc.set_option("count_visits", 1)
        return sc, closer

    twin, close_twin = make()
    for rv in RVS[:5]:
        twin.render_frame(*rv)
    want_sum, want_stats, want_count = frames_state(twin, depth)
    close_twin()
    sc, closer = make()
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    stats3, count3 = sc.frame_stats(), sc.frame_count
    sc.render_aov(*RVS[0])
    sc.denoise(1.0 / 3.0)
    aov, denoised = read_all(cr, sc), sc.read_denoised()
    p = sc.resolve_device(1.0 / 3.0)
    rgba, sum3 = device_bytes_at(p, W * H * 4), sc.read_sum()
    sc.temporal(1.0 / 3.0, clamp=True)
    sc.temporal(1.0 / 3.0, clamp=True)
    sc.resolve_temporal_device()
    n2 = sc.read_temporal_history()
    assert n2.max() == 2 or abs(n2.max() - 2) < 1e-5
    assert sc.frame_stats() == stats3 and sc.frame_count == count3
    assert np.array_equal(sc.read_sum().view(np.uint32), sum3.view(np.uint32))
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(words(after[n]), words(aov[n])), n
    assert np.array_equal(sc.read_denoised().view(np.uint32), denoised.view(np.uint32))
    assert np.array_equal(device_bytes_at(p, W * H * 4), rgba)
    for rv in RVS[3:5]:
        sc.render_frame(*rv)
    got_sum, got_stats, got_count = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats and got_count == want_count and got_stats["closest_rays"] > 0
    sc.reset()                                                 # the sum goes, the history stays
    assert np.array_equal(sc.read_temporal_history().view(np.uint32), n2.view(np.uint32))
    closer()


@pytest.mark.gpu
def test_g5_refusals_leave_image_and_history_as_they_were(cr, ob, cornell, textured):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError, crt_temporal_params
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[0]
    L = _lib.lib()
    buf = np.zeros(W * H * 12, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    d, view = directions(ob, cam, W, H, RVS[0]), view_record(cam, W, H)

    def refused(call):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == CRT_ERR_INVALID, e.value
        assert str(e.value).split(": ", 1)[1]                 # crt_last_error says why

    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:2])
    for call in (sc.read_temporal, sc.read_temporal_history, sc.temporal_device, sc.resolve_temporal, sc.resolve_temporal_device, lambda: sc.temporal(0.5)):
        refused(call)
    for missing in ("HIT", "IDS", "NORMAL", "ALBEDO"):
        sc2 = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
        sc2.render_aov(*RVS[0], channels=cr.AOV_ALL & ~bit_of(cr, missing))
        refused(lambda: sc2.temporal(0.5))
        if missing == "ALBEDO":
            sc2.temporal(0.5, demodulate=False)               # ALBEDO is needed by DEMODULATE alone
        else:
            refused(lambda: sc2.temporal(0.5, demodulate=False))
            refused(sc2.read_temporal)
        sc2.close()
    sc.render_aov(*RVS[0], channels=cr.AOV_ALL & ~cr.AOV_EMISSION)
    state, _ = check_call(cr, ob, sc, None, d, view, None, None, "G5 first", 1, 32, inv=0.5)
    state, _ = check_call(cr, ob, sc, state, d, view, None, None, "G5 second", 1, 32, inv=0.5)
    want_image, want_n = sc.read_temporal(), sc.read_temporal_history()

    def raw(inv=0.5, **fields):
        p = crt_temporal_params()
        p.flags, p.source, p.max_history, p.sigma_depth, p.normal_min = 1, 0, 32, 0.1, 0.9
        for k, v in fields.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return lambda: _lib.check(L.crt_temporal(sc._h, inv, C.byref(p), 1))

    nan, inf = float("nan"), float("inf")
    calls = [raw(inv=0.0), raw(inv=-1.0), raw(inv=nan), raw(inv=inf), raw(flags=4), raw(flags=7), raw(flags=1 << 31), raw(source=2), raw(source=1),
             raw(max_history=0), raw(max_history=4097), raw(sigma_depth=0.0), raw(sigma_depth=-0.1), raw(sigma_depth=1e-7), raw(sigma_depth=2e6),
             raw(sigma_depth=nan), raw(sigma_depth=inf), raw(normal_min=-1.5), raw(normal_min=1.5), raw(normal_min=nan), raw(normal_min=inf),
             raw(reserved=0), raw(reserved=1), raw(reserved=2),
             lambda: _lib.check(L.crt_read_temporal(sc._h, ptr, W * H * 3 - 3)), lambda: _lib.check(L.crt_read_temporal(sc._h, ptr, W * H * 4)),
             lambda: _lib.check(L.crt_read_temporal_history(sc._h, ptr, W * H - 1)), lambda: _lib.check(L.crt_read_temporal_history(sc._h, ptr, W * H * 3)),
             lambda: _lib.check(L.crt_resolve_temporal(sc._h, ptr, W * H * 4 - 4)), lambda: _lib.check(L.crt_resolve_temporal(sc._h, ptr, W * H * 3)),
             lambda: sc.set_option("temporal_form", 3)]
    for k, call in enumerate(calls):
        refused(call)
        assert np.array_equal(sc.read_temporal().view(np.uint32), want_image.view(np.uint32)), k
        assert np.array_equal(sc.read_temporal_history().view(np.uint32), want_n.view(np.uint32)), k
    assert L.crt_temporal_device(sc._h, None) == CRT_ERR_INVALID and L.crt_resolve_temporal_device(sc._h, None, 1) == CRT_ERR_INVALID
    assert not buf.any()
    # a shard of the frame and a scene on several devices are refused; both restart the sum, not the history
    sc.set_shard(0, 2, 16)
    refused(lambda: sc.temporal(0.5))
    sc.set_shard(0, 1, 16)
    sc.set_devices([0, 0])
    refused(lambda: sc.temporal(0.5))
    sc.set_devices([0])
    assert np.array_equal(sc.read_temporal_history().view(np.uint32), want_n.view(np.uint32))
    sc.reset()
    sc.render_frames(RVS[:2])
    # the history is as it was: a valid call still matches the reference, which was given the state from before the refusals
    state, cs = check_call(cr, ob, sc, state, d, view, None, None, "G5 after the refusals", 1, 32, inv=0.5)
    assert cs["with_history"] > 0
    # NULL params are the spelled-out defaults
    want, want_n, state, _ = temporal_ref(state, (sc.read_sum() * f32(0.5)).astype(f32), {n: sc.read_aov(bit_of(cr, n)) for n in GUIDES}, d, view, None, None, params_of(1))
    _lib.check(L.crt_temporal(sc._h, 0.5, None, 1))
    assert np.array_equal(sc.read_temporal().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sc.read_temporal_history().view(np.uint32), want_n.view(np.uint32))
    # the edges of the ranges are accepted
    raw(max_history=1, sigma_depth=1e-6, normal_min=-1.0)()
    raw(max_history=4096, sigma_depth=1e6, normal_min=1.0, flags=3)()
    # sync = 0 and a read give what sync = 1 gives
    sc.temporal_reset()
    sc.temporal(0.5, sync=True)
    sc.temporal(0.5, clamp=True, sync=True)
    a_image, a_n, a_rgba = sc.read_temporal(), sc.read_temporal_history(), sc.resolve_temporal()
    sc.temporal_reset()
    sc.temporal(0.5, sync=False)
    sc.temporal(0.5, clamp=True, sync=False)
    assert np.array_equal(sc.read_temporal().view(np.uint32), a_image.view(np.uint32))
    assert np.array_equal(sc.read_temporal_history().view(np.uint32), a_n.view(np.uint32)) and np.array_equal(sc.resolve_temporal(), a_rgba)
    assert a_n.max() > 1
    # a toggle of DEMODULATE and a reset: N = 1 everywhere
    sc.temporal(0.5, demodulate=False)
    assert (sc.read_temporal_history() == 1).all()
    sc.temporal(0.5, demodulate=False)
    assert sc.read_temporal_history().max() > 1
    sc.temporal_reset()
    sc.temporal(0.5, demodulate=False)
    assert (sc.read_temporal_history() == 1).all()
    sc.temporal(0.5, sync=False)
    sc.resolve_temporal_device(sync=False)
    sc.close()                                                 # destroy with the calls still queued


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g6_ten_calls_hold_the_memory_of_the_first(cr, cornell, textured, kind):
    W, H = DENOISE_SIZES[1]
    if kind == "flat":
        mesh, _ = flat_variants(cr, cornell, textured)["textured"]
        sc = flat_scene(cr, mesh, cornell[1], "sbvh", W, H, 3)
        inst = None
    else:
        _, inst, sc = walls_handle(cr, W, H)
    sc.render_frames(RVS[:2])
    sc.render_aov(*RVS[0])
    used0 = device_bytes_in_use()
    used = []
    for k in range(10):
        sc.temporal(0.5, demodulate=bool(k & 2), clamp=bool(k & 1), max_history=1 + k)
        sc.resolve_temporal_device()
        sc.read_temporal_history()
        used.append(device_bytes_in_use())
    print("device bytes in use after each temporal:", used, "the first call took", used[0] - used0)
    assert all(u == used[1] for u in used[1:]), used
    sc.close()
    if inst:
        inst.close()


@pytest.mark.gpu
def test_g7_the_three_resolves_share_staging_not_buffers(cr, cornell, textured):
    """32 x 24 Cornell box, one frame, render_aov, denoise, temporal: the host resolves of the sum, the denoised and the accumulated image
    go through one pinned staging buffer, each from a device buffer of its own.  Read once each, then again in reverse order with a device
    resolve between each pair: every host image equals its first reading byte for byte, the three device pointers are pairwise distinct"""
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    W, H = 32, 24
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", W, H, 3)
    sc.render_frame(*RVS[0])
    sc.render_aov(*RVS[0])
    sc.denoise(1.0)
    sc.temporal(1.0)
    first = [sc.resolve(1.0), sc.resolve_denoised(), sc.resolve_temporal()]
    for img in first:
        assert img.shape == (H, W, 4) and img[..., :3].any()
    again, pointers = [None, None, None], []
    again[2] = sc.resolve_temporal()
    pointers.append(sc.resolve_device(1.0))
    again[1] = sc.resolve_denoised()
    pointers.append(sc.resolve_temporal_device())
    again[0] = sc.resolve(1.0)
    pointers.append(sc.resolve_denoised_device())
    for name, a, b in zip(("sum", "denoised", "temporal"), first, again):
        assert np.array_equal(a, b), name
    assert all(pointers) and len(set(pointers)) == 3, pointers
    sc.close()
