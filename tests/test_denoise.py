"""crt_denoise: the edge-avoiding a-trous filter over the running sum, guided by the first-hit feature buffers, held BY
BYTES to tests/denoise_ref.py, the definition in float32 numpy.  The reference's inputs are the handle's own read_sum() and read_aov(),
which other tests hold to the oracle, so each check isolates the filter.

CPU: the ABI and the Python surface (C1), the premises the GPU checks rest on (C2: every way a tap can be cut or weighted occurs in the
test frames), the quality of the definition (C3).  GPU: flat scenes (G1), instanced scenes across a refit (G2), nothing else moves (G3),
ordering (G4), refusals and lifetime (G5).  No tolerance anywhere: the expected number of differing words is 0."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest

from denoise_ref import denoise_ref, filterable
from test_aov import (CHANNELS, bit_of, device_bytes_at, flat_data, flat_reference, flat_scene, frames_state, general_handle, identity_scene,
                      instanced_reference, offsets_for, read_all, words)
from test_instances_frames import RVS, flat_variants, look_at, primary_oracle, shading_of
from test_instances_oracle import host_blas, host_scene, is_identity, orc

f32 = np.float32
SIZES = ((67, 45), (231, 130))
SMALL = (20, 9)
NAMES = ["cornell", "textured", "tess8_mat"]
ENTRIES = ("crt_denoise", "crt_read_denoised", "crt_denoised_device", "crt_resolve_denoised", "crt_resolve_denoised_device")
ISSUE = dict(passes=5, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7)
CLASSES = ("edge", "unfilterable", "normal_zero", "normal_partial", "depth_zero", "depth_partial", "color_zero", "color_partial")


def guides(aov):
    return {n: aov[n] for n in ("HIT", "IDS", "NORMAL", "ALBEDO")}


# ---------------------------------------------------------------- the two-walls scene of C2 / G2 ----

def two_walls(cr):
    """one flat wall mesh (a 2 x 2 quad in z = 0) placed twice side by side, x in [-2, 0] and [0, 2]: coplanar, the same normal, depth
    continuous across the seam, so the KEY alone separates the two; each instance its own Lambert albedo through its material offset"""
    quad = cr.Mesh(np.array([[-1, -1, 0], [1, -1, 0], [1, 1, 0], [-1, 1, 0]], f32), np.array([[0, 0, 1]], f32), np.zeros((0, 2), f32),
                   np.array([[0, 1, 2, 0, 0, 0, 0, 1, 0, 0, 0, 0], [0, 2, 3, 0, 0, 0, 0, 1, 0, 0, 0, 0]], np.int32), np.zeros((1, 16), f32), np.zeros((0, 18), f32))
    table = np.zeros((2, 16), f32)
    table[:, 7], table[:, 12:16] = -1, -1
    table[0, :3], table[1, :3] = (0.8, 0.3, 0.2), (0.2, 0.4, 0.9)
    M = np.array([[[1, 0, 0, -1], [0, 1, 0, 0], [0, 0, 1, 0]], [[1, 0, 0, 1], [0, 1, 0, 0], [0, 0, 1, 0]]], f32)
    # the light: a 6 x 6 quad at z = 6 that faces the walls
    light = np.concatenate([(-3, -3, 6), (6, 0, 0), (0, 6, 0), (0, 0, -1), (40, 40, 40), (36.0, 0.5, 0)]).astype(f32)[None]
    return dict(meshes=[quad], table=table, M=M, mesh_of=np.array([0, 0]), offs=np.array([0, 1], np.uint32), light=light)


def camera_w(cr):
    return look_at(cr, (0.0, 0.0, 4.0), (0.0, 0.0, 0.0))


# ---------------------------------------------------------------- C1 ----

def test_c1_header_exports_and_binding_agree(cr, cornell_data):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crt.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    raw = C.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in _lib.SYMBOLS and hasattr(raw, name) and hasattr(L, name), name
    assert re.search(r"CRT_DENOISE_DEMODULATE = 1\b", code) and _lib.CRT_DENOISE_DEMODULATE == 1 == _lib.DENOISE_DEMODULATE
    assert C.sizeof(_lib.crt_denoise_params) == 32
    fields = re.search(r"typedef struct crt_denoise_params \{(.*?)\} crt_denoise_params;", code, flags=re.S).group(1)
    assert re.findall(r"(\w+)(?:\[\d+\])?;", fields) == [n for n, _ in _lib.crt_denoise_params._fields_]
    assert L.crt_abi_version() == 6
    for name in ("denoise", "read_denoised", "denoised_device", "resolve_denoised", "resolve_denoised_device"):
        assert callable(getattr(cr.Scene, name))
    sig = inspect.signature(cr.Scene.denoise)
    assert [(k, p.default) for k, p in sig.parameters.items()][1:] == [("inv_count", None), ("passes", 5), ("demodulate", True), ("sigma_color", 4.0),
                                                                         ("sigma_depth", 0.05), ("normal_power_log2", 7), ("sync", True)]
    assert inspect.signature(cr.Scene.resolve_denoised_device).parameters["sync"].default is True
    # a null scene is refused before anything else, with a reason
    buf = np.zeros(16, np.uint8)
    p = C.c_void_p()
    ptr = buf.ctypes.data_as(C.c_void_p)
    assert L.crt_denoise(None, 1.0, None, 1) == _lib.CRT_ERR_INVALID and b"null" in L.crt_last_error()
    assert L.crt_read_denoised(None, ptr, 4) == _lib.CRT_ERR_INVALID
    assert L.crt_denoised_device(None, C.byref(p)) == _lib.CRT_ERR_INVALID and not p.value
    assert L.crt_resolve_denoised(None, ptr, 16) == _lib.CRT_ERR_INVALID
    assert L.crt_resolve_denoised_device(None, C.byref(p), 1) == _lib.CRT_ERR_INVALID and not p.value
    if L.crt_device_count() == 0:                              # no scene exists without a device: no CPU fallback
        with pytest.raises(cr.CrtError) as e:
            cr.Scene(cornell_data, 64, 64, 1)
        assert e.value.code == _lib.CRT_ERR_NO_DEVICE


# ---------------------------------------------------------------- C2, C3: on the oracle ----

_ORACLE = {}


def oracle_inputs(cr, ob, cornell, W, H, n_frames, depth=3):
    """(sum of the oracle's first n_frames RVS frames, the guides of RVS[0]'s primary rays) of the Cornell box, computed once per case"""
    key = (W, H, n_frames, depth)
    if key not in _ORACLE:
        mesh, cam = cornell
        data = flat_data(cr, mesh, cam, "sbvh")
        o = ob.Oracle(data, W, H, depth, camera=cam)
        total = np.zeros((H, W, 3), f32)
        for rv in RVS[:n_frames]:
            o.render_frame(rv[0], rv[1], total, threads=16)
        _ORACLE[key] = (total, guides(flat_reference(cr, ob, "cornell", "sbvh", mesh, data, cam, W, H, RVS[0], 1)))
    return _ORACLE[key]


def test_c2_every_way_a_tap_is_cut_or_weighted_occurs(cr, ob, cornell):
    """Measured here (Cornell, 4 oracle frames, guides of the first RVS pair jittered), (filterable pixel, off-centre tap) pairs:
    67 x 45, 48,192 pairs in every pass.  s = 1: 1,205 edge; 1,803 unfilterable; 6,746 / 7,254 normal zero / partial; 11,004 / 34,156 depth
    zero / partial; 1,216 / 43,064 colour zero / partial.  s = 2: 2,570 edge; 3,080 unfilterable; 10,482 / 7,462 normal; 9,819 / 32,701 depth;
    1,376 / 41,150 colour.  s = 4: 5,230 edge; 5,278 unfilterable; 15,936 / 7,300 normal; 5,412 / 32,252 depth; 1,516 / 36,158 colour.
    20 x 9, s = 16: 1,824 of 1,824 pairs cut by the frame edge.  Two walls at 67 x 45, s = 1: 27,984 pairs, 2,264 unfilterable, 720 cut by
    the key alone, none by the normal or the depth term."""
    W, H = SIZES[0]
    total, aov = oracle_inputs(cr, ob, cornell, W, H, 4)
    out, census = denoise_ref(total, aov, 0.25, **ISSUE)
    assert np.isfinite(out).all()
    for i in range(3):
        print(f"C2 {W}x{H} s = {1 << i}:", census[i])
        assert census[i]["pairs"] == 24 * int(filterable(aov).sum()) > 0
        assert census[i]["key"] == 0                           # a flat scene has one key: the two walls below carry that class
        for name in CLASSES:
            assert census[i][name] > 0, (i, name, census[i])
    W, H = SMALL
    total, aov = oracle_inputs(cr, ob, cornell, W, H, 4)
    out, census = denoise_ref(total, aov, 0.25, **ISSUE)
    print(f"C2 {W}x{H} s = 16:", census[4])
    assert census[4]["pairs"] > 0 and census[4]["edge"] == census[4]["pairs"]
    F = filterable(aov)
    assert np.array_equal(out[~F].view(np.uint32), (total * f32(0.25)).astype(f32)[~F].view(np.uint32))
    # an instanced scene: the key alone cuts pairs (the same plane, the same normal, continuous depth across the seam)
    w = two_walls(cr)
    W, H = SIZES[0]
    s = host_scene(cr, [host_blas(cr, m) for m in w["meshes"]], list(w["M"]), list(w["mesh_of"]))
    rays = primary_oracle(ob, camera_w(cr), W, H).primary_rays(*RVS[0], jitter=True)
    hits, ids, _, _, refused = orc(ob, s, rays)
    assert refused.sum() == 0
    w2o = np.array([cr.instance_inverse(m) for m in w["M"]], f32).reshape(-1, 3, 4)
    ident = np.array([is_identity(m) for m in w["M"]])
    ref = instanced_reference(cr, W, H, rays, hits, ids, w["meshes"], w["mesh_of"], w["offs"], w["table"], None, w2o, ident)
    _, census = denoise_ref(np.zeros((H, W, 3), f32), guides(ref), 1.0, passes=1, demodulate=True, sigma_color=0.0, sigma_depth=0.05, normal_power_log2=7)
    print(f"C2 two walls {W}x{H} s = 1:", census[0])
    assert census[0]["key"] > 0 and census[0]["unfilterable"] > 0
    assert census[0]["normal_zero"] == 0 and census[0]["normal_partial"] == 0 and census[0]["depth_zero"] == 0       # nothing but the key separates the walls
    assert set(np.unique(ref["IDS"]["instance"])) == {-1, 0, 1}


def test_c3_the_definition_removes_noise(cr, ob, cornell):
    """Cornell at 96 x 64, max_depth 3, against 256 oracle frames; 3 passes, sigma_color 4, sigma_depth 0.05, power 2^7, demodulated.
    Measured here: MSE(denoised) / MSE(noisy) = 0.368 at 1 frame, 0.467 at 4 frames (bound 0.6, a property of the definition)."""
    W, H = 96, 64
    mesh, cam = cornell
    data = flat_data(cr, mesh, cam, "sbvh")
    o = ob.Oracle(data, W, H, 3, camera=cam)
    rng = np.random.default_rng(2024)
    ref = np.zeros((H, W, 3), f32)
    for rx, ry in rng.uniform(0.0, 1.0, (256, 2)):
        o.render_frame(rx, ry, ref, threads=16)
    ref = ref.astype(np.float64) / 256.0
    for n in (1, 4):
        total, aov = oracle_inputs(cr, ob, cornell, W, H, n)
        inv = f32(1.0 / n)
        out, _ = denoise_ref(total, aov, inv, passes=3, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7)
        noisy = (total * inv).astype(f32)
        assert np.isfinite(out).all()
        F = filterable(aov)
        assert 0 < (~F).sum() < F.size
        assert np.array_equal(out[~F].view(np.uint32), noisy[~F].view(np.uint32))
        mse_noisy, mse_out = np.mean((noisy - ref) ** 2), np.mean((out - ref) ** 2)
        print(f"C3 {n} frame(s): MSE noisy {mse_noisy:.5g}, denoised {mse_out:.5g}, ratio {mse_out / mse_noisy:.3f}")
        assert mse_out <= 0.6 * mse_noisy


# ---------------------------------------------------------------- GPU ----

def check_denoise(cr, ob, sc, inv, what, **kw):
    """one crt_denoise against the definition on the handle's own sum and guides, by bytes; returns the reference image"""
    want, _ = denoise_ref(sc.read_sum(), {n: sc.read_aov(bit_of(cr, n)) for n in ("HIT", "IDS", "NORMAL", "ALBEDO")}, inv, **kw)
    sc.denoise(inv, **kw)
    got = sc.read_denoised()
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(2))
    print(f"{what} {kw}: pixels with a differing word: {bad[0].size}")
    assert bad[0].size == 0, (what, kw, bad[0].size, bad[0][:4], bad[1][:4], got[bad][:4], want[bad][:4])
    assert np.array_equal(sc.resolve_denoised(), ob.resolve(want, 1.0)), (what, kw)
    return want


def device_bytes_in_use():
    """through the HIP runtime the library itself is linked to, as device_bytes_at reads"""
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)
    hip.hipMemGetInfo.argtypes = [C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    hip.hipMemGetInfo.restype = C.c_int
    free, total = C.c_size_t(), C.c_size_t()
    assert hip.hipMemGetInfo(C.byref(free), C.byref(total)) == 0
    return total.value - free.value


def check_device_pointers(sc, want_image, want_rgba):
    W, H = sc.width, sc.height
    p = sc.denoised_device()
    assert p and np.array_equal(device_bytes_at(p, W * H * 12), np.ascontiguousarray(want_image).view(np.uint8).reshape(-1))
    q = sc.resolve_denoised_device()
    assert q and np.array_equal(device_bytes_at(q, W * H * 4), np.ascontiguousarray(want_rgba).reshape(-1))


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_g1_flat_scenes_by_bytes(cr, ob, cornell, textured, name):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    inv = f32(0.25)
    for W, H in SIZES + (SMALL,):
        sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
        sc.set_option("jitter", 1)
        sc.render_frames(RVS[:4])
        sc.render_aov(*RVS[0])
        F = filterable(guides(read_all(cr, sc)))
        assert 0 < F.sum() < F.size
        if (W, H) == SMALL:
            want = check_denoise(cr, ob, sc, inv, f"G1 {name} {W}x{H}", **ISSUE)
        else:
            for passes in (1, 3, 5):
                for demodulate in (True, False):
                    for sigma_color in (0.0, 4.0):
                        want = check_denoise(cr, ob, sc, inv, f"G1 {name} {W}x{H}", passes=passes, demodulate=demodulate, sigma_color=sigma_color,
                                             sigma_depth=0.05, normal_power_log2=7)
            if (W, H) == SIZES[1]:
                want = check_denoise(cr, ob, sc, inv, f"G1 {name} {W}x{H}", passes=6, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7)
            # the product runs each pass in the form measured faster at its spacing; here each form at EVERY spacing (option "denoise_form")
            for form in (1, 2):
                sc.set_option("denoise_form", form)
                for kw in (dict(ISSUE, passes=6 if (W, H) == SIZES[1] else 5), dict(ISSUE, passes=3, demodulate=False, sigma_color=0.0)):
                    want = check_denoise(cr, ob, sc, inv, f"G1 {name} {W}x{H} form {form}", **kw)
            sc.set_option("denoise_form", 0)
        check_device_pointers(sc, want, ob.resolve(want, 1.0))
        sc.close()


def walls_handle(cr, W, H, depth=3):
    w = two_walls(cr)
    inst = cr.InstancedScene(w["meshes"], cr.instances_array(w["M"], w["mesh_of"], material_offsets=w["offs"]))
    sc = inst.frame_scene(shading_of(w["meshes"]), w["table"], w["light"], W, H, depth)
    sc.update(camera_w(cr))
    return w, inst, sc


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["general", "walls"])
def test_g2_instanced_scenes_before_and_after_a_refit(cr, ob, cornell, tess8, kind):
    inv = f32(0.25)
    if kind == "general":
        g, inst, sc, cam = general_handle(cr, cornell, tess8)
        M2 = g["M"].copy()
        M2[:, :, 3] += g["rng"].uniform(-1.5, 1.5, (120, 3)).astype(f32)
        moved = cr.instances_array(M2, g["mesh_of"], g["masks"], offsets_for(g["rng"], g["meshes"], g["mesh_of"], g["table"].shape[0]))
    else:
        w, inst, sc = walls_handle(cr, *SIZES[0])
        M2 = w["M"].copy()
        M2[:, :, 3] += np.array([[0.25, 0.5, -0.5], [-0.125, -0.25, 0.75]], f32)
        moved = cr.instances_array(M2, w["mesh_of"], material_offsets=w["offs"])
    seen = []
    for step in ("created", "refitted"):
        if step == "refitted":
            inst.refit(moved)
            sc.reset()
        sc.render_frames(RVS[:4])
        sc.render_aov(*RVS[0])
        aov = read_all(cr, sc)
        assert len(set(np.unique(aov["IDS"]["instance"])) - {-1}) >= 2          # more than one key in view
        for kw in (ISSUE, dict(ISSUE, passes=3, demodulate=False), dict(ISSUE, passes=1, sigma_color=0.0)):
            want = check_denoise(cr, ob, sc, inv, f"G2 {kind} {step}", **kw)
        check_device_pointers(sc, want, ob.resolve(want, 1.0))
        seen.append(aov["HIT"])
    assert (words(seen[0]) != words(seen[1])).any()                               # the refit moved what the camera sees
    if kind == "walls":
        _, census = denoise_ref(sc.read_sum(), guides(aov), inv, **dict(ISSUE, passes=1))
        assert census[0]["key"] > 0
    sc.close()
    inst.close()


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g3_nothing_else_moves(cr, ob, cornell, textured, kind, depth):
    """3 frames, render_aov, denoise, resolve_denoised, 2 frames: the sum and the stats of 5 frames alone (at max_depth 3 without the four
    wave-level step counts that follow the queue order, test_aov G7's rule); every AOV channel and crt_resolve_device's buffer keep their bytes"""
    mesh, parts = flat_variants(cr, cornell, textured)["tess8_mat"]
    cam = cornell[1]
    W, H = SIZES[1]

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

    plain, close_plain = make()
    for rv in RVS[:5]:
        plain.render_frame(*rv)
    want_sum, want_stats, want_count = frames_state(plain, depth)
    close_plain()
    sc, closer = make()
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    stats3 = sc.frame_stats()
    sc.render_aov(*RVS[0])
    aov = read_all(cr, sc)
    p = sc.resolve_device(1.0 / 3.0)
    rgba = device_bytes_at(p, W * H * 4)
    sum3 = sc.read_sum()
    want = check_denoise(cr, ob, sc, f32(1.0 / 3.0), f"G3 {kind} depth {depth}", **ISSUE)
    check_device_pointers(sc, want, ob.resolve(want, 1.0))
    assert sc.frame_stats() == stats3
    assert np.array_equal(sc.read_sum().view(np.uint32), sum3.view(np.uint32))
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(words(after[n]), words(aov[n])), n
    assert np.array_equal(device_bytes_at(p, W * H * 4), rgba)
    assert (rgba.reshape(-1, 4) != sc.resolve_denoised().reshape(-1, 4)).any()          # and the two images are not the same picture
    for rv in RVS[3:5]:
        sc.render_frame(*rv)
    got_sum, got_stats, got_count = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats and got_count == want_count
    assert got_stats["closest_rays"] > 0
    closer()


@pytest.mark.gpu
def test_g4_enqueued_behind_async_frames_and_aovs(cr, ob, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[1]
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:4])
    sc.render_aov(*RVS[1])
    sc.denoise(0.25, **ISSUE)
    want_image, want_rgba = sc.read_denoised(), sc.resolve_denoised()
    sc.close()
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:4], sync=False)
    sc.render_aov(*RVS[1], sync=False)
    sc.denoise(0.25, sync=False, **ISSUE)
    q = sc.resolve_denoised_device(sync=True)
    assert np.array_equal(device_bytes_at(q, W * H * 4), want_rgba.reshape(-1))
    assert np.array_equal(sc.read_denoised().view(np.uint32), want_image.view(np.uint32))
    # later frames are ordered behind it, and crt_sync waits for it
    total4, aov = sc.read_sum(), guides(read_all(cr, sc))
    sc.denoise(0.25, sync=False, **dict(ISSUE, passes=2))
    sc.render_frame(*RVS[4], sync=False)
    sc.sync()
    want2, _ = denoise_ref(total4, aov, 0.25, **dict(ISSUE, passes=2))
    assert np.array_equal(sc.read_denoised().view(np.uint32), want2.view(np.uint32))
    assert (sc.read_sum().view(np.uint32) != total4.view(np.uint32)).any()
    sc.close()


@pytest.mark.gpu
def test_g5_refusals_leave_the_denoised_image_as_it_was(cr, ob, cornell, textured):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError, crt_denoise_params
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[0]
    L = _lib.lib()
    buf = np.zeros(W * H * 12, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    dev = C.c_void_p()

    def refused(call):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == CRT_ERR_INVALID, e.value
        assert str(e.value).split(": ", 1)[1]                 # crt_last_error says why

    # before any crt_denoise, and before the guides exist
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:4])
    for call in (sc.read_denoised, sc.denoised_device, sc.resolve_denoised, sc.resolve_denoised_device, lambda: sc.denoise(0.25)):
        refused(call)
    for missing in ("HIT", "IDS", "NORMAL", "ALBEDO"):
        sc2 = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
        sc2.render_aov(*RVS[0], channels=cr.AOV_ALL & ~bit_of(cr, missing))
        refused(lambda: sc2.denoise(0.25))
        refused(sc2.read_denoised)
        sc2.close()
    sc.render_aov(*RVS[0], channels=cr.AOV_ALL & ~cr.AOV_EMISSION)                 # EMISSION is not needed
    want = check_denoise(cr, ob, sc, f32(0.25), "G5", **ISSUE)
    rgba = sc.resolve_denoised()
    # NULL params are the spelled-out defaults
    _lib.check(L.crt_denoise(sc._h, 0.25, None, 1))
    assert np.array_equal(sc.read_denoised().view(np.uint32), want.view(np.uint32))

    def raw(inv=0.25, **fields):
        p = crt_denoise_params()
        p.passes, p.flags, p.sigma_color, p.sigma_depth, p.normal_power_log2 = 5, 1, 4.0, 0.05, 7
        for k, v in fields.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return lambda: _lib.check(L.crt_denoise(sc._h, inv, C.byref(p), 1))

    nan, inf = float("nan"), float("inf")
    calls = [raw(inv=0.0), raw(inv=-1.0), raw(inv=nan), raw(inv=inf), raw(passes=0), raw(passes=7), raw(flags=2), raw(flags=3), raw(flags=1 << 31),
             raw(reserved=0), raw(reserved=1), raw(reserved=2), raw(sigma_color=-1.0), raw(sigma_color=1e-7), raw(sigma_color=2e6), raw(sigma_color=nan),
             raw(sigma_color=inf), raw(sigma_depth=0.0), raw(sigma_depth=-0.05), raw(sigma_depth=1e-7), raw(sigma_depth=2e6), raw(sigma_depth=nan),
             raw(sigma_depth=inf), raw(normal_power_log2=11),
             lambda: _lib.check(L.crt_read_denoised(sc._h, ptr, W * H * 3 - 3)), lambda: _lib.check(L.crt_read_denoised(sc._h, ptr, W * H * 4)),
             lambda: _lib.check(L.crt_resolve_denoised(sc._h, ptr, W * H * 4 - 4)), lambda: _lib.check(L.crt_resolve_denoised(sc._h, ptr, W * H * 3))]
    # the image on the device, through pointers taken BEFORE the refusals: read after each one, before any accepted call could rewrite it
    p_image, p_rgba = sc.denoised_device(), sc.resolve_denoised_device()
    want_bytes, rgba_bytes = np.ascontiguousarray(want).view(np.uint8).reshape(-1), np.ascontiguousarray(rgba).reshape(-1)

    def image_is_as_it_was(what):
        assert np.array_equal(device_bytes_at(p_image, W * H * 12), want_bytes), what
        assert np.array_equal(device_bytes_at(p_rgba, W * H * 4), rgba_bytes), what

    image_is_as_it_was("before")
    calls.append(lambda: sc.set_option("denoise_form", 3))
    for k, call in enumerate(calls):
        refused(call)
        image_is_as_it_was(("refusal", k))
    assert L.crt_denoised_device(sc._h, None) == CRT_ERR_INVALID and L.crt_resolve_denoised_device(sc._h, None, 1) == CRT_ERR_INVALID
    assert not buf.any()
    image_is_as_it_was("null pointers")
    assert np.array_equal(sc.read_denoised().view(np.uint32), want.view(np.uint32)) and np.array_equal(sc.resolve_denoised(), rgba)
    # "a channel never rendered" cannot be met by a handle that holds an image: the channels a scene has rendered only grow, and an image
    # needs all four.  A partial render_aov on such a handle keeps the other channels' contents, and the call is accepted
    sc.render_aov(*RVS[0], channels=cr.AOV_HIT)
    sc.denoise(0.25)                                          # the same sum, the same guides: the same image
    image_is_as_it_was("the same view's HIT again")
    # a shard of the frame and a scene on several devices lack the neighbours
    sc.set_shard(0, 2, 16)
    refused(lambda: sc.denoise(0.25))
    image_is_as_it_was("shard")
    sc.set_shard(0, 1, 16)
    sc.set_devices([0, 0])
    refused(lambda: sc.denoise(0.25))
    image_is_as_it_was("two devices")
    sc.set_devices([0])
    image_is_as_it_was("one device again")
    assert np.array_equal(sc.read_denoised().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(sc.resolve_denoised(), rgba)
    check_device_pointers(sc, want, rgba)
    # the edges of the ranges are accepted, and the defaults give the image back
    raw(passes=1, sigma_color=0.0, normal_power_log2=0)()
    assert not np.array_equal(device_bytes_at(p_image, W * H * 12), want_bytes)
    raw(passes=6, sigma_color=1e6, sigma_depth=1e6, normal_power_log2=10)()
    sc.reset()                                                # set_shard and set_devices restarted the sum: the same four frames again
    sc.render_frames(RVS[:4])
    raw()()
    image_is_as_it_was("defaults again")
    sc.close()


@pytest.mark.gpu
def test_g5_ten_calls_hold_the_memory_of_the_first_and_destroy_after_async(cr, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[1]
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H, 3)
    sc.render_frames(RVS[:4])
    sc.render_aov(*RVS[0])
    used0 = device_bytes_in_use()
    sc.denoise(0.25)
    sc.resolve_denoised_device()
    used = []
    for k in range(10):
        sc.denoise(0.25, passes=1 + k % 6, demodulate=bool(k & 1))
        sc.resolve_denoised_device()
        used.append(device_bytes_in_use())
    print("device bytes in use after each denoise:", used, "the first call took", used[0] - used0)
    assert all(u == used[0] for u in used), used
    sc.denoise(0.25, sync=False)
    sc.resolve_denoised_device(sync=False)
    sc.close()                                                 # destroy with the call still queued
