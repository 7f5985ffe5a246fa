"""Fog with light shafts (crt_render_fog, crt_fog_segments, crt_fog_composite) held bit for bit to tests/fog_ref.py, a float32
numpy restatement of the definition in include/crt.h whose occlusion is a brute force over every triangle.

CPU: the ABI (C1), exp_neg by its own properties (C2), the premise of the GPU checks — the oracle's CWBVH any-hit walk and the brute force
agree on EVERY fog ray of every flat case, and the cases are not trivial (C3) —, values that need no reference (C4), and the mistakes the
scenes must notice (C5).  GPU: flat views (G1), the definition through crt_trace_device (G2), segments mode (G3), the sample counts at the
word boundaries (G4), instanced scenes (G5), nothing else moves (G6), the composite and its display (G7), refusals and lifetime (G8).  All
pixels and all four words are compared; there is no tolerance.

The flat cases look at the Cornell box from outside its left wall towards its open front: pixels that miss everything, pixels whose whole
segment lies in the wall's shadow, pixels that look into the lit box, and the shadow's edge between them."""
import ctypes as C
import math
import types

import numpy as np
import pytest

import display_ref as dr
import fog_ref
from test_ao import device_array, frames_state
from test_aov import CHANNELS, device_bytes_at, flat_data, flat_scene, identity_scene, read_all
from test_instanced_ref import MASKS_ON, open_scene, ref_scene, with_new_lamp_lights, yard
from test_instances_frames import RVS, flat_variants
from test_lens import lens_camera

f32 = np.float32
THREADS = 16
SMALL, LARGE = (67, 45), (231, 130)
CASES = [("cornell", SMALL), ("cornell", LARGE), ("textured", SMALL), ("textured", LARGE), ("tess8_mat", SMALL)]   # tess8's size bounds the brute force
K1 = 8
RV = RVS[0]
MAX_DISTANCE = 12.0
THIN, THICK = 0.08, 20.0      # at 20 per unit, sigma * (s + ln) passes 104 on most samples: exp_neg's +0
ALBEDO, AMBIENT = (0.9, 0.8, 0.7), (0.02, 0.03, 0.05)
MEDIA = [(g, density) for g in (0.0, 0.6) for density in (THIN, THICK)]


def params(K=K1, density=THIN, g=0.0, max_distance=MAX_DISTANCE, albedo=ALBEDO, ambient=AMBIENT):
    return fog_ref.Params(K=K, density=density, albedo=albedo, anisotropy=g, max_distance=max_distance, ambient=ambient)


def kwargs(p):
    return dict(samples=p.K, density=p.density, albedo=p.albedo, anisotropy=p.anisotropy, max_distance=p.max_distance, ambient=p.ambient)


def segment_kwargs(p):
    kw = kwargs(p)
    del kw["max_distance"]
    return kw


def words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1, 4)


def assert_words(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], np.asarray(got).reshape(-1, 4)[bad[:4]], np.asarray(want).reshape(-1, 4)[bad[:4]])


def look_at(position, target, fov):
    """a camera at `position` looking at `target`, y up"""
    from caitlynrenderer_amd._lib import crt_camera
    pos, at = np.asarray(position, np.float64), np.asarray(target, np.float64)
    forward = (at - pos) / np.linalg.norm(at - pos)
    right = np.cross(forward, [0.0, 1.0, 0.0])
    right /= np.linalg.norm(right)
    up = np.cross(right, forward)
    c = crt_camera()
    for name, v in (("position", pos), ("right", right), ("up", up), ("forward", forward)):
        for i in range(3):
            getattr(c, name)[i] = float(f32(v[i]))
    c.fov, c.focal_dist, c.aperture = fov, 0.1, 0.0
    return types.SimpleNamespace(c=c)


@pytest.fixture(scope="module")
def side(cornell):
    return look_at((-4.0, 2.75, 9.0), (1.0, 2.2, 3.0), cornell[1].fov)


_REF = {}


def flat_ref(cr, cornell, textured, cam, name, size, jitter, p=None, breaks=()):
    """(image (H, W, 4), rays) of a flat case, computed once and never written again; the occlusion answers of a view are shared by its media"""
    p = params() if p is None else p
    key = (name, size, jitter, p, tuple(breaks))
    if key not in _REF:
        mesh, _ = flat_variants(cr, cornell, textured)[name]
        scene = fog_ref.RefScene(mesh, cam, *size)
        base = (name, size, jitter, params(K=p.K, max_distance=p.max_distance), ())
        known = None if breaks or key == base else flat_ref(cr, cornell, textured, cam, name, size, jitter, base[3])[1]
        img, rays = fog_ref.render_fog(scene, RV[0], RV[1], p, jitter=jitter, breaks=breaks, known=known)
        img.setflags(write=False)
        _REF[key] = (img, rays)
    return _REF[key]


# ---------------------------------------------------------------- C1 ----

def test_c1_the_entries_are_exported_and_refuse_null_scenes(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    names = ("crt_render_fog", "crt_read_fog", "crt_fog_device", "crt_fog_segments", "crt_fog_segments_device", "crt_fog_composite",
             "crt_read_fogged", "crt_fogged_device", "crt_display_fogged")
    for name in names:
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert cr.FOG_SEGMENT_DT.itemsize == 32 and cr.FOG_SEGMENT_DT.names == ("o", "seed_x", "e", "seed_y")
    assert cr.FOG_SEGMENT_DT == fog_ref.FOG_SEGMENT_DT
    assert C.sizeof(_lib.crt_fog_params) == 64
    buf = np.zeros(8, f32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = C.c_void_p()
    null = lambda rc: rc == _lib.CRT_ERR_INVALID and b"null" in L.crt_last_error()
    assert null(L.crt_render_fog(None, 0.0, 0.0, None, 1))
    assert null(L.crt_read_fog(None, ptr, 8))
    assert null(L.crt_fog_device(None, C.byref(p))) and not p.value
    assert null(L.crt_fog_segments(None, ptr, 1, 0.0, 0.0, None, ptr))
    assert null(L.crt_fog_segments_device(None, ptr, 1, 0.0, 0.0, None, ptr, 1))
    assert null(L.crt_fog_composite(None, 1.0, 0, 1))
    assert null(L.crt_read_fogged(None, ptr, 8))
    assert null(L.crt_fogged_device(None, C.byref(p))) and not p.value
    assert null(L.crt_display_fogged(None, None, 1))
    assert not buf.any()
    assert L.crt_abi_version() == 6
    for name in ("render_fog", "read_fog", "fog_device", "fog_segments", "fog_segments_device", "fog_composite", "read_fogged", "fogged_device",
                 "display_fogged"):
        assert callable(getattr(cr.Scene, name))


# ---------------------------------------------------------------- C2: exp_neg by its own properties ----

def test_c2_exp_neg_is_within_an_ulp_monotone_and_exact_at_its_ends():
    rng = np.random.default_rng(17)
    tiny = np.array([0.0, 1e-45, 1e-40, 1.1754942e-38, 1e-30], f32)
    x = np.sort(np.concatenate([rng.uniform(0.0, 104.0, 100000).astype(f32), tiny, f32([103.9, 104.0, 1e30])]))
    got = fog_ref.exp_neg(x)
    want = np.array([math.exp(-float(v)) for v in x], np.float64).astype(f32)        # the correctly rounded value, but for double's own 1e-16
    # distance in units of the last place: the floats of one sign are ordered like their bit patterns
    ulps = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64))
    print("C2: worst distance from exp(-x) rounded to float32, in ulps:", int(ulps.max()), "at", x[ulps.argmax()])
    assert ulps.max() <= 1
    assert (np.diff(got.astype(np.float64)) <= 0).all()
    assert got[0] == 1.0 and x[0] == 0.0
    assert (fog_ref.exp_neg(tiny) == 1.0).all()
    beyond = fog_ref.exp_neg(f32([104.0, 104.00001, 1e30, np.inf]))
    assert (beyond.view(np.uint32) == 0).all()                                       # +0, not -0
    assert fog_ref.exp_neg(f32([103.9]))[0] > 0
    assert (got[x >= THICK * 6.0] < 1e-37).any() and (got == 0).any()


# ---------------------------------------------------------------- C3: the premise of the GPU checks ----

def lit_counts(rays, K):
    n = rays["add"].sum(1)
    return dict(miss=int((rays["tri"] < 0).sum()), all=int((n == K).sum()), none=int((n == 0).sum()), part=int(((n > 0) & (n < K)).sum()))


@pytest.mark.parametrize("name,size", CASES)
def test_c3_the_oracle_walk_and_the_brute_force_agree_on_every_ray(cr, ob, cornell, textured, side, name, size):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    orc = ob.Oracle(flat_data(cr, mesh, side, "sbvh"), size[0], size[1], 1, camera=side)
    for jitter in (0, 1):
        img, r = flat_ref(cr, cornell, textured, side, name, size, jitter)
        idx = np.nonzero(r["lit"])
        rays = np.zeros(idx[0].size, cr.RAY_DT)
        rays["o"], rays["d"], rays["tmax"] = r["x"][idx], r["ld"][idx], r["tmax"][idx]
        hit = orc.trace(rays, ob.BVH8, ob.ANY, ob.TIE_LOWEST_ID, threads=THREADS)["tri"] >= 0
        disagree = int((hit != ~r["visible"][idx]).sum())
        counts = lit_counts(r, K1)
        print(f"C3 {name} {size} jitter {jitter}: rays {rays.shape[0]}, dark samples {int((~r['lit']).sum())}, disagreements {disagree}, pixels {counts}")
        assert disagree == 0
        assert min(counts.values()) > 0, counts
        assert r["ok"].all()
        thick = flat_ref(cr, cornell, textured, side, name, size, jitter, params(density=THICK))[0]
        assert (thick[..., 3] == 0).any() and (words(thick) != words(img)).any()


# ---------------------------------------------------------------- C4: values that need no reference ----

def test_c4_no_density_no_fog_and_no_lights_only_ambient(cr, cornell, textured, side):
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    scene = fog_ref.RefScene(mesh, side, *SMALL)
    known = flat_ref(cr, cornell, textured, side, "cornell", SMALL, 1)[1]
    clear = fog_ref.render_fog(scene, RV[0], RV[1], params(density=0.0), known=known)[0]
    assert (clear == f32([0, 0, 0, 1])).all()
    dark = fog_ref.RefScene(mesh, side, *SMALL, lights=np.zeros((0, 18), f32))
    for density in (THIN, THICK):
        img = fog_ref.render_fog(dark, RV[0], RV[1], params(density=density))[0]
        TD = img[..., 3]
        want = (f32(AMBIENT) * f32(ALBEDO)).astype(f32)[None, None, :] * (f32(1.0) - TD)[..., None]
        assert np.array_equal(img[..., :3].view(np.uint32), want.astype(f32).view(np.uint32))
        assert (TD < 1).all()


def open_scene_with_one_light(cam):
    """nothing between the fog and its light: one far, tiny triangle (a scene needs one) and one light overhead, facing down"""
    V = np.array([[500, 500, 500], [500.01, 500, 500], [500, 500.01, 500]], f32)
    tri = np.zeros((1, 12), np.int32)
    tri[0, :3], tri[0, 4:8] = (0, 1, 2), (0, 1, 0, 0)
    mats = np.zeros((1, 16), f32)
    mats[0, 7] = mats[0, 12] = -1
    light = np.zeros((1, 18), f32)
    light[0, 0:3], light[0, 3:6], light[0, 6:9], light[0, 9:12] = (-0.5, 3.0, -0.5), (1, 0, 0), (0, 0, 1), (0, -1, 0)
    light[0, 12:15], light[0, 15], light[0, 16] = (5.0, 4.0, 3.0), 1.0, 1.0
    mesh = types.SimpleNamespace(vertices=V, normals=np.zeros((0, 3), f32), texcoords=np.zeros((0, 2), f32), triangles=tri, materials=mats, lights=light)
    return fog_ref.RefScene(mesh, cam, 8, 8)


def test_c4_eight_and_sixty_four_strata_estimate_the_same_mean(cornell):
    scene = open_scene_with_one_light(cornell[1])
    rng = np.random.default_rng(23)
    seg = np.zeros(256, fog_ref.FOG_SEGMENT_DT)
    seg["o"], seg["e"] = (-2.0, 0.5, 0.3), (4.0, 0.4, -0.2)                         # passes under the light
    seg["seed_x"], seg["seed_y"] = rng.uniform(0.5, 2000, 256), rng.uniform(0.5, 2000, 256)
    S = {}
    for K in (8, 64):
        out, r = fog_ref.fog_segments(scene, seg, *RV, params(K=K, density=0.3, ambient=(0, 0, 0)))
        assert r["add"].all()                                                        # nothing occludes, nothing is dark
        S[K] = out[:, :3].astype(np.float64)
    se = np.sqrt(S[8].var(0, ddof=1) / 256 + S[64].var(0, ddof=1) / 256)
    z = np.abs(S[8].mean(0) - S[64].mean(0)) / se
    print("C4: means at K = 8 and 64:", S[8].mean(0), S[64].mean(0), "apart by standard errors:", z)
    assert (S[8].mean(0) > 0).all() and (z <= 4).all()


# ---------------------------------------------------------------- C5: the mistakes the scenes must notice ----

@pytest.fixture(scope="module")
def yard_scene(cr, textured):
    return yard(cr, textured[0].albedo_textures)


YARD_P = params(g=0.6, max_distance=9.0)
_YARD = {}


def yard_ref(s, options, key, p=YARD_P, breaks=(), rv=RV, lights=None):
    k = (key, p, tuple(breaks), rv)
    if k not in _YARD:
        scene = ref_scene(s, options)
        img, rays = fog_ref.render_fog(scene, rv[0], rv[1], p, jitter=1, breaks=breaks, lights=lights)
        img.setflags(write=False)
        _YARD[k] = (img, rays, scene.lights)
    return _YARD[k]


@pytest.mark.parametrize("brk", fog_ref.BREAKS)
def test_c5_a_mistake_in_the_reference_changes_words(cr, cornell, textured, side, yard_scene, brk):
    p = params(g=0.6)
    want = flat_ref(cr, cornell, textured, side, "cornell", SMALL, 1, p)[0]
    got = flat_ref(cr, cornell, textured, side, "cornell", SMALL, 1, p, breaks=(brk,))[0]
    diff = int((words(got) != words(want)).sum())
    diff_y = int((words(yard_ref(yard_scene, None, "Y", breaks=(brk,))[0]) != words(yard_ref(yard_scene, None, "Y")[0])).sum())
    print(f"C5 {brk}: differing words on cornell {diff}, on the yard {diff_y}")
    assert diff > 0 and diff_y > 0


# ---------------------------------------------------------------- G1: flat views ----

@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sbvh", "sah"])
@pytest.mark.parametrize("name,size", CASES)
def test_g1_flat_views_bit_for_bit(cr, cornell, textured, side, name, size, builder):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    sc = flat_scene(cr, mesh, side, builder, *size)
    for jitter in (0, 1):
        sc.set_option("jitter", jitter)
        for g, density in MEDIA:
            p = params(g=g, density=density)
            want = flat_ref(cr, cornell, textured, side, name, size, jitter, p)[0]
            sc.render_fog(*RV, **kwargs(p))
            assert_words(sc.read_fog(), want, (name, size, builder, jitter, g, density))
    assert sc.frame_stats()["stack_overflows"] == 0
    sc.close()


# ---------------------------------------------------------------- G2: the definition itself ----

def fold_of_a_trace(cr, trace_device, r, p, mode, pad=None):
    """the reference's rays through a crt_trace_device-like entry (ANY), folded in numpy"""
    import torch
    idx = np.nonzero(r["lit"])
    n = idx[0].size
    rays = np.zeros(n, cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = r["x"][idx], r["ld"][idx], r["tmax"][idx]
    if pad is not None:
        rays["pad"] = pad
    d_rays, d_hits = device_array(rays), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    trace_device(d_rays.data_ptr(), n, d_hits.data_ptr(), mode=mode)
    add = np.zeros(r["lit"].shape, bool)
    add[idx] = d_hits.cpu().numpy().view(cr.HIT_DT)["tri"] < 0
    return fog_ref.fold(r["ok"], r["D"], r["contrib"], add, p)


@pytest.mark.gpu
@pytest.mark.parametrize("density", [THIN, THICK])
def test_g2_the_rays_through_crt_trace_device_fold_to_the_same_bytes(cr, cornell, textured, side, density):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    p = params(g=0.6, density=density)
    _, r = flat_ref(cr, cornell, textured, side, "textured", LARGE, 1, p)
    sc = flat_scene(cr, mesh, side, "sbvh", *LARGE)
    sc.render_fog(*RV, **kwargs(p))
    assert_words(sc.read_fog(), fold_of_a_trace(cr, sc.trace_device, r, p, cr.CRT_TRACE_ANY), ("trace_device", density))
    sc.close()


# ---------------------------------------------------------------- G3: segments mode ----

@pytest.mark.gpu
def test_g3_segments_mode_gives_the_views_bytes(cr, cornell, textured, side):
    import torch
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    p = params(g=0.6)
    want, r = flat_ref(cr, cornell, textured, side, "textured", LARGE, 1, p)
    want = want.reshape(-1, 4)
    seg = r["segments"]
    kw = segment_kwargs(p)
    sc = flat_scene(cr, mesh, side, "sbvh", *LARGE)
    got = sc.fog_segments(seg, *RV, **kw)                                         # the whole view, miss pixels included
    assert_words(got, want, "host form, the view")
    d_seg, d_out = device_array(seg), torch.zeros(seg.shape[0] * 16, dtype=torch.uint8, device="cuda")
    sc.fog_segments_device(d_seg.data_ptr(), seg.shape[0], d_out.data_ptr(), *RV, **kw)
    assert_words(d_out.cpu().numpy().view(f32), want, "device form, the view")
    part = np.nonzero((r["add"].sum(1) > 0) & (r["add"].sum(1) < K1))[0]            # the shadow's edge
    for n in (1, 63, 64, 65, 515):                                                # 515 x 8 entries: beyond 4096, and several pools of 256
        idx = part[7:7 + n]
        assert idx.size == n
        assert_words(sc.fog_segments(seg[idx], *RV, **kw), want[idx], ("n", n))
        d_part, d_res = device_array(seg[idx]), torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        sc.fog_segments_device(d_part.data_ptr(), n, d_res.data_ptr(), *RV, **kw)
        assert_words(d_res.cpu().numpy().view(f32), want[idx], ("n on the device", n))
    # n = 0 succeeds and writes nothing
    assert sc.fog_segments(seg[:0], *RV, **kw).shape == (0, 4)
    sc.fog_segments_device(0, 0, 0, *RV, **kw)
    # segments without rays between segments with: (0, 0, 0, -1), the neighbours right
    idx = part[100:107]
    odd = seg[idx].copy()
    odd["e"][1] = 0
    odd["e"][3] = (np.nan, 1, 0)
    odd["o"][5] = (np.inf, 0, 0)
    expect = want[idx].copy()
    expect[[1, 3, 5]] = (0, 0, 0, -1)
    assert_words(sc.fog_segments(odd, *RV, **kw), expect, "segments without rays")
    d_odd, d_res = device_array(odd), torch.zeros(7 * 16, dtype=torch.uint8, device="cuda")
    sc.fog_segments_device(d_odd.data_ptr(), 7, d_res.data_ptr(), *RV, **kw)
    assert_words(d_res.cpu().numpy().view(f32), expect, "segments without rays, on the device")
    # segments of the caller's own against the reference
    scene = fog_ref.RefScene(mesh, side, *LARGE)
    rng = np.random.default_rng(5)
    mine = np.zeros(64, fog_ref.FOG_SEGMENT_DT)
    mine["o"] = rng.uniform(0.5, 5.0, (64, 3))
    mine["e"] = rng.uniform(-3.0, 3.0, (64, 3))
    mine["seed_x"], mine["seed_y"] = rng.uniform(0.5, 500, 64), rng.uniform(0.5, 500, 64)
    q = params(K=16, density=0.4, g=-0.5)
    ref, rr = fog_ref.fog_segments(scene, mine, *RVS[1], q)
    assert rr["add"].any() and not rr["add"].all()
    assert_words(sc.fog_segments(mine, *RVS[1], **segment_kwargs(q)), ref, "free segments")
    sc.close()


# ---------------------------------------------------------------- G4: K at the word boundaries ----

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 31, 32, 33, 256])
def test_g4_sample_counts_at_the_word_boundaries(cr, cornell, textured, side, K):
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    p = params(K=K, g=0.6)
    want = flat_ref(cr, cornell, textured, side, "cornell", SMALL, 1, p)[0]
    sc = flat_scene(cr, mesh, side, "sbvh", *SMALL)
    sc.render_fog(*RV, **kwargs(p))
    assert_words(sc.read_fog(), want, K)
    sc.close()


# ---------------------------------------------------------------- G5: instanced scenes ----

@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_g5_identity_instances_give_the_flat_scenes_bytes(cr, cornell, textured, side, builder):
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    inst, sc, _ = identity_scene(cr, mesh, parts, builder, *SMALL)
    sc.update(side)
    for g, density in MEDIA:
        p = params(g=g, density=density)
        want = flat_ref(cr, cornell, textured, side, "textured", SMALL, 1, p)[0]
        sc.render_fog(*RV, **kwargs(p))
        assert_words(sc.read_fog(), want, (builder, g, density))
    sc.close()
    inst.close()


def yard_check(cr, inst, sc, s, options, key, what, ray_mask=None):
    """the scene's image against the reference over the table the scene reports, and against the handle's own trace of the reference's rays"""
    table = cr.read_lights(sc)
    want, r, own = yard_ref(s, options, key, lights=table)
    assert np.array_equal(table.view(np.uint32), own.view(np.uint32)), what       # the table the reference builds by itself
    sc.render_fog(*RV, **kwargs(YARD_P))
    got = sc.read_fog()
    assert_words(got, want, what)
    mode = cr.CRT_TRACE_ANY | (0 if ray_mask is None else cr.CRT_TRACE_INSTANCE_MASK)
    assert_words(got, fold_of_a_trace(cr, inst.trace_device, r, YARD_P, mode, ray_mask), (what, "the handle's trace"))
    return want, r


@pytest.mark.gpu
def test_g5_a_lit_yard_across_a_refit_and_new_mesh_lights(cr, textured, yard_scene):
    y = yard_scene
    moved = yard(cr, textured[0].albedo_textures, moved=True)
    inst, sc = open_scene(cr, y, 1)
    want, r = yard_check(cr, inst, sc, y, None, "Y", "created")
    counts = lit_counts(r, K1)
    print("G5 yard:", counts, "dark samples", int((~r["lit"]).sum()))
    assert min(counts.values()) > 0 and (~r["lit"]).any()
    inst.refit(cr.instances_array(moved.M, moved.mesh_of, masks=moved.masks, material_offsets=moved.offsets))     # seen by the next call, no crt_reset
    want2, _ = yard_check(cr, inst, sc, moved, None, "Y'", "refitted")
    assert (words(want2) != words(want)).any()
    relit = with_new_lamp_lights(moved)
    cr.set_mesh_lights(sc, 3, relit.mesh_lights[3])
    want3, _ = yard_check(cr, inst, sc, relit, None, "Y' relit", "new mesh lights")
    assert (words(want3) != words(want2)).any()
    sc.close()
    inst.close()


@pytest.mark.gpu
def test_g5_mask_shadow_hides_an_occluder(cr, yard_scene):
    y = yard_scene
    inst, sc = open_scene(cr, y, 1, options=MASKS_ON)
    masked, _ = yard_check(cr, inst, sc, y, MASKS_ON, "Y masked", "masked", MASKS_ON["mask_shadow"])
    sc.set_option("mask_shadow", 0xff)
    seen, _ = yard_check(cr, inst, sc, y, {**MASKS_ON, "mask_shadow": 0xff}, "Y masked, shadow rays see all", "mask_shadow 255", 0xff)
    changed = (words(masked) != words(seen)).any(1)
    print("G5 masks: pixels the hidden occluder changes:", int(changed.sum()))
    assert changed.any()
    sc.set_option("instance_masks", 0)
    plain, _ = yard_check(cr, inst, sc, y, None, "Y", "option back to 0")
    assert (words(plain) != words(masked)).any()
    sc.close()
    inst.close()


# ---------------------------------------------------------------- G6: nothing else moves ----

@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g6_a_call_between_frames_changes_nothing_else(cr, cornell, textured, side, kind, depth):
    mesh, parts = flat_variants(cr, cornell, textured)["tess8_mat"]
    W, H = LARGE
    p = params(g=0.6)

    def make():
        if kind == "flat":
            sc = flat_scene(cr, mesh, side, "sbvh", W, H, depth)
            closer = sc.close
        else:
            inst, sc, _ = identity_scene(cr, mesh, parts, "sah", W, H, depth)
            sc.update(side)
            closer = lambda: (sc.close(), inst.close())
        sc.set_option("count_visits", 1)
        return sc, closer

    plain, close_plain = make()
    for rv in RVS[:5]:
        plain.render_frame(*rv)
    want_sum, want_stats, want_count = frames_state(plain, depth)
    plain.render_fog(*RVS[3], **kwargs(p))
    want_fog = plain.read_fog()
    assert (want_fog[..., :3] > 0).any()
    close_plain()
    sc, closer = make()
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    stats3 = sc.frame_stats()
    sc.render_aov(*RVS[2])
    aov = read_all(cr, sc)
    sc.render_ao(*RVS[2], samples=4)
    ao = sc.read_ao()
    sc.render_fog(*RVS[3], **kwargs(p))
    assert_words(sc.read_fog(), want_fog, "between frames")
    assert sc.frame_stats() == stats3
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(np.ascontiguousarray(after[n]).view(np.uint8), np.ascontiguousarray(aov[n]).view(np.uint8)), n
    assert_words(sc.read_ao(), ao, "the AO image")
    for rv in RVS[3:5]:
        sc.render_frame(*rv)
    got_sum, got_stats, got_count = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats and got_count == want_count
    closer()
    # enqueued without a host wait behind asynchronous frames, a frame behind it
    sc, closer = make()
    sc.render_frames(RVS[:3], sync=False)
    sc.render_fog(*RVS[3], sync=False, **kwargs(p))
    for rv in RVS[3:5]:
        sc.render_frame(*rv, sync=False)
    sc.sync()
    assert_words(sc.read_fog(), want_fog, "async")
    got_sum, got_stats, _ = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32)) and got_stats == want_stats
    closer()


@pytest.mark.gpu
def test_g6_a_lens_and_an_environment_change_no_byte(cr, cornell, textured, side):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    want = flat_ref(cr, cornell, textured, side, "textured", SMALL, 1)[0]
    sc = flat_scene(cr, mesh, side, "sbvh", *SMALL)
    sc.update(lens_camera(cr, side, 0.05, 3.0))
    sc.render_fog(*RV, **kwargs(params()))
    assert_words(sc.read_fog(), want, "lens")
    sc.set_environment(cr.constant_environment((0.5, 0.7, 1.0)))
    sc.render_fog(*RV, **kwargs(params()))
    assert_words(sc.read_fog(), want, "lens and environment")
    sc.close()


# ---------------------------------------------------------------- G7: the composite ----

def bits3(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


@pytest.mark.gpu
def test_g7_the_composite_on_every_source_and_its_display(cr, cornell, textured, side):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    sc = flat_scene(cr, mesh, side, "sbvh", *LARGE, 3)
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    inv = f32(1.0 / 3.0)
    sc.render_aov(*RVS[2])
    sc.denoise(inv, passes=2)
    sc.temporal(inv, source="sum")
    images = {"sum": (sc.read_sum(), inv), "denoised": (sc.read_denoised(), None), "temporal": (sc.read_temporal(), None)}
    p = params(g=0.6)
    fog = flat_ref(cr, cornell, textured, side, "textured", LARGE, 1, p)[0]
    seen = set()
    for density in (THIN, 0.0):
        q = params(g=0.6, density=density) if density else params(g=0.6, density=0.0, ambient=(0, 0, 0))
        sc.render_fog(*RV, **kwargs(q))
        if density:
            assert_words(sc.read_fog(), fog, "the fog under the composite")
        for source, (image, inv_count) in images.items():
            assert not np.signbit(image[image == 0]).any()                        # the sources here have no negative zeros
            sc.fog_composite(inv if inv_count is None else inv_count, source=source)
            got = sc.read_fogged()
            c = image if inv_count is None else (image * inv_count).astype(f32)
            if density:
                want = fog_ref.composite(image, fog, inv_count)
                assert np.array_equal(bits3(got), bits3(want)), source
                assert (bits3(got) != bits3(c)).any()
                seen.add(got.tobytes())
            else:
                assert np.array_equal(bits3(got), bits3(c)), source               # no fog: the source pixel's bits
            ptr = sc.fogged_device()
            assert np.array_equal(device_bytes_at(ptr, got.nbytes), got.view(np.uint8).reshape(-1))
            assert np.array_equal(bits3(sc.read_sum()), bits3(images["sum"][0]))
    assert len(seen) == 3
    # a segment without rays keeps the source pixel: the reference's rule on a made-up fog image
    holed = np.array(fog)
    holed[::2, ::3] = (0, 0, 0, -1)
    want = fog_ref.composite(images["denoised"][0], holed)
    assert np.array_equal(bits3(want[::2, ::3]), bits3(images["denoised"][0][::2, ::3]))
    # the display of the fogged image: display_ref on the image read back; a metered call and a manual one after it
    sc.render_fog(*RV, **kwargs(p))
    sc.fog_composite(inv, source="sum")
    fogged = sc.read_fogged()
    meter = dr.Meter()
    sc.display_reset()
    for dp in (dr.Params(source="denoised", curve="aces", auto=True, adapt=0.5), dr.Params(source="denoised", curve="reinhard", exposure=0.5, white=2.0)):
        want, state, hist = dr.display(fogged, f32(1.0), dp, meter)                 # "denoised": the image as it is
        kw = dp.kwargs()
        del kw["source"]
        got = sc.display_fogged(**kw)
        st = sc.display_state()
        assert (st["counted"], st["q"], st["calls"]) == (state["counted"], state["q"], state["calls"]), (st, state)
        assert bits3(st["metered"]) == bits3(state["metered"]) and bits3(st["exposure"]) == bits3(state["exposure"]), (st, state)
        if dp.auto:
            assert sc.display_histogram().tolist() == hist
        assert np.array_equal(got, want)
    assert np.array_equal(bits3(sc.read_fogged()), bits3(fogged))
    sc.close()


# ---------------------------------------------------------------- G8: refusals and lifetime ----

@pytest.mark.gpu
def test_g8_refusals_name_the_field_and_leave_the_images(cr, cornell, textured, side):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    W, H = SMALL
    want = flat_ref(cr, cornell, textured, side, "textured", SMALL, 1)[0]
    sc = flat_scene(cr, mesh, side, "sbvh", W, H)
    L = _lib.lib()

    def refused(call, word):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == CRT_ERR_INVALID and word in str(e.value), (word, e.value)

    refused(lambda: sc.read_fog(), "no crt_render_fog")                           # reads and a composite before any render
    refused(lambda: sc.fog_device(), "no crt_render_fog")
    refused(lambda: sc.fog_composite(1.0), "no crt_render_fog")
    sc.render_frame(*RV)
    sum_before = sc.read_sum()
    sc.render_fog(*RV, **kwargs(params()))
    assert_words(sc.read_fog(), want, "first")
    refused(lambda: sc.read_fogged(), "no crt_fog_composite")                     # reads and a display before any composite
    refused(lambda: sc.fogged_device(), "no crt_fog_composite")
    refused(lambda: sc.display_fogged(), "no crt_fog_composite")
    refused(lambda: sc.fog_composite(1.0, source="denoised"), "no crt_denoise")   # sources that do not exist
    refused(lambda: sc.fog_composite(1.0, source="temporal"), "no crt_temporal")
    refused(lambda: _lib.check(L.crt_fog_composite(sc._h, 1.0, 3, 1)), "source")
    for inv in (0.0, -1.0, float("nan"), float("inf")):
        refused(lambda: sc.fog_composite(inv), "inv_count")
    sc.fog_composite(1.0)
    fogged = sc.read_fogged()
    assert np.array_equal(bits3(fogged), bits3(fog_ref.composite(sum_before, want, f32(1.0))))
    seg = np.zeros(4, cr.FOG_SEGMENT_DT)
    seg["e"] = (0, 1, 0)
    out = np.full((4, 4), 7, f32)

    def raw(**kw):
        p = _lib.crt_fog_params()
        p.samples, p.flags, p.density, p.anisotropy, p.max_distance = 16, 0, 0.05, 0.0, 100.0
        p.albedo[:] = (1.0, 1.0, 1.0)
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            elif k in ("albedo", "ambient"):
                getattr(p, k)[v[0]] = v[1]
            else:
                setattr(p, k, v)
        return p

    def entries(p):
        ptr, optr = seg.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        return [lambda: _lib.check(L.crt_render_fog(sc._h, 0.3, 0.8, C.byref(p), 1)),
                lambda: _lib.check(L.crt_fog_segments(sc._h, ptr, 4, 0.3, 0.8, C.byref(p), optr)),
                lambda: _lib.check(L.crt_fog_segments_device(sc._h, ptr, 4, 0.3, 0.8, C.byref(p), optr, 1))]

    nan, inf = float("nan"), float("inf")
    bad = [(dict(samples=0), "samples"), (dict(samples=257), "samples"), (dict(flags=1), "flags"), (dict(reserved=0), "reserved"), (dict(reserved=4), "reserved"),
           (dict(density=-1e-6), "density"), (dict(density=2e6), "density"), (dict(density=nan), "density"), (dict(density=inf), "density"),
           (dict(albedo=(0, -0.1)), "albedo"), (dict(albedo=(1, 1.1)), "albedo"), (dict(albedo=(2, nan)), "albedo"),
           (dict(anisotropy=-1.0), "anisotropy"), (dict(anisotropy=0.995), "anisotropy"), (dict(anisotropy=nan), "anisotropy"),
           (dict(max_distance=0.0), "max_distance"), (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=inf), "max_distance"),
           (dict(max_distance=nan), "max_distance"),
           (dict(ambient=(0, -0.1)), "ambient"), (dict(ambient=(1, inf)), "ambient"), (dict(ambient=(2, nan)), "ambient")]
    for kw, word in bad:
        for call in entries(raw(**kw)):
            refused(call, word)
    ptr, optr = seg.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    refused(lambda: _lib.check(L.crt_fog_segments(sc._h, None, 4, 0.3, 0.8, None, optr)), "null")
    refused(lambda: _lib.check(L.crt_fog_segments(sc._h, ptr, 4, 0.3, 0.8, None, None)), "null")
    refused(lambda: _lib.check(L.crt_fog_segments_device(sc._h, None, 4, 0.3, 0.8, None, optr, 1)), "null")
    refused(lambda: _lib.check(L.crt_fog_segments_device(sc._h, ptr, 4, 0.3, 0.8, None, None, 1)), "null")
    p256 = raw(samples=256)
    refused(lambda: _lib.check(L.crt_fog_segments_device(sc._h, ptr, 1 << 24, 0.3, 0.8, C.byref(p256), optr, 1)), "2^32")      # n * K = 2^32
    refused(lambda: _lib.check(L.crt_fog_segments(sc._h, ptr, 1 << 24, 0.3, 0.8, C.byref(p256), optr)), "2^32")
    buf = np.zeros(W * H * 4, f32)
    refused(lambda: _lib.check(L.crt_read_fog(sc._h, buf.ctypes.data_as(C.c_void_p), W * H * 4 - 4)), "n_floats")
    refused(lambda: _lib.check(L.crt_read_fog(sc._h, buf.ctypes.data_as(C.c_void_p), W * H * 3)), "n_floats")
    refused(lambda: _lib.check(L.crt_read_fogged(sc._h, buf.ctypes.data_as(C.c_void_p), W * H * 4)), "n_floats")
    dp = _lib.crt_display_params()
    dp.source, dp.exposure, dp.white = 1, 1.0, 4.0
    refused(lambda: _lib.check(L.crt_display_fogged(sc._h, C.byref(dp), 1)), "source")
    sc.set_option("accel", 1)
    for call in entries(raw()):
        refused(call, "accel")
    sc.set_option("accel", 0)
    assert (out == 7).all() and not buf.any()
    assert_words(sc.read_fog(), want, "after the refusals")
    assert np.array_equal(bits3(sc.read_fogged()), bits3(fogged))
    assert np.array_equal(sc.read_sum().view(np.uint32), sum_before.view(np.uint32))
    p = sc.fog_device()
    assert p and np.array_equal(device_bytes_at(p, W * H * 16), np.ascontiguousarray(want).view(np.uint8).reshape(-1))
    sc.set_devices([0, 0])                                     # two logical devices behind the handle
    for call in entries(raw()):
        refused(call, "one device")
    refused(lambda: sc.fog_composite(1.0), "one device")
    sc.set_devices([0])
    assert_words(sc.read_fog(), want, "after set_devices")
    sc.set_option("streams", 2)                                # the frame's tiles dealt to two streams of the one device
    for call in entries(raw()):
        refused(call, "one stream")
    refused(lambda: sc.fog_composite(1.0), "one stream")
    sc.set_option("streams", 1)
    assert_words(sc.read_fog(), want, "after option streams")
    sc.render_fog(*RV, **kwargs(params()))
    assert_words(sc.read_fog(), want, "on one stream again")
    sc.close()
    # a scene that never had a camera has no view to march
    blind = cr.Scene(cr.SceneData.build(mesh, None), W, H, 1)
    refused(lambda: blind.render_fog(*RV), "crt_set_camera")
    refused(lambda: blind.read_fog(), "no crt_render_fog")
    blind.update(side)
    blind.render_fog(*RV, **kwargs(params()))
    assert_words(blind.read_fog(), want, "once it has one")
    blind.close()
    # a shard of a frame; a frame too large for 32-bit entry indices
    sc = flat_scene(cr, mesh, side, "sbvh", W, H)
    sc.set_shard(1, 2, 16)
    for call in entries(raw()):
        refused(call, "crt_set_shard")
    sc.close()
    big = flat_scene(cr, mesh, side, "sbvh", 8192, 4096)
    refused(lambda: big.render_fog(*RV, samples=128), "2^32")                     # 2^25 pixels x 2^7
    big.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g8_ten_calls_hold_the_memory_of_the_first(cr, cornell, textured, side, kind):
    import torch
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    if kind == "flat":
        sc, inst = flat_scene(cr, mesh, side, "sbvh", *LARGE), None
    else:
        inst, sc, _ = identity_scene(cr, mesh, parts, "sah", *LARGE)
        sc.update(side)
    sc.render_frame(*RV)
    used = []
    for k in range(10):
        sc.render_fog(*RVS[k % 8], **kwargs(params()))
        sc.fog_composite(1.0)
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
    print("device bytes in use after each render_fog + fog_composite:", used)
    assert all(u == used[0] for u in used), used
    sc.close()
    if inst is not None:
        inst.close()


@pytest.mark.gpu
def test_g8_after_rebuild_vertices_the_image_shows_the_new_positions(cr, cornell, textured, side):
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    rng = np.random.default_rng(5)
    moved = cr.Mesh((mesh.vertices + rng.uniform(-0.15, 0.15, mesh.vertices.shape)).astype(f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials,
                    mesh.lights, mesh.vertex_min)
    sc = flat_scene(cr, mesh, side, "sah", *SMALL)
    sc.render_fog(*RV, **kwargs(params()))
    before = flat_ref(cr, cornell, textured, side, "cornell", SMALL, 1)[0]
    assert_words(sc.read_fog(), before, "built")
    sc.rebuild_vertices(moved.vertices)
    sc.render_fog(*RV, **kwargs(params()))
    want = fog_ref.render_fog(fog_ref.RefScene(moved, side, *SMALL), RV[0], RV[1], params())[0]
    assert_words(sc.read_fog(), want, "rebuilt")
    assert (words(want) != words(before)).any()
    sc.close()
