"""Ambient occlusion (crt_render_ao, crt_ao_points) held bit for bit to tests/ao_ref.py, a float32 numpy restatement of
the definition in include/crt.h whose occlusion is a brute force over every triangle.

CPU: the ABI (C1), the sampler by its own properties (C2), the premise of the GPU checks — the oracle's CWBVH any-hit walk and the brute
force agree on EVERY occlusion ray of every flat case, and the cases are not trivial (C3) —, the analytic ends (C4), and the mistakes the
scenes must notice (C5).  GPU: flat views (G1), the definition through crt_trace_device (G2), points mode (G3), the sample counts at the
word boundaries (G4), instanced scenes (G5), nothing else moves (G6), refusals and lifetime (G7).  All points and all four words are
compared; there is no tolerance."""
import ctypes as C
import types

import numpy as np
import pytest

import ao_ref
from test_aov import CHANNELS, device_bytes_at, flat_data, flat_scene, identity_scene, read_all
from test_instanced_ref import MASKS_ON, open_scene, ref_scene, yard
from test_instances_frames import RVS, flat_variants
from test_lens import lens_camera

f32 = np.float32
THREADS = 16
SMALL, LARGE = (67, 45), (231, 130)
CASES = [("cornell", SMALL), ("cornell", LARGE), ("textured", SMALL), ("textured", LARGE), ("tess8_mat", SMALL)]   # tess8's size bounds the brute force
K1 = 8
RV = RVS[0]
BOUNDED = f32(0.35)           # of the scene's largest extent


def words(a):
    return np.ascontiguousarray(a, f32).view(np.uint32).reshape(-1, 4)


def assert_words(got, want, what):
    g, w = words(got), words(want)
    bad = np.nonzero((g != w).any(1))[0]
    assert bad.size == 0, (what, bad.size, bad[:4], np.asarray(got).reshape(-1, 4)[bad[:4]], np.asarray(want).reshape(-1, 4)[bad[:4]])


def radius_of(mesh, bounded):
    if not bounded:
        return ao_ref.UNBOUNDED
    V = mesh.vertices[mesh.triangles[:, :3].reshape(-1)]
    return f32(BOUNDED * f32((V.max(0) - V.min(0)).max()))


_REF = {}


def flat_ref(cr, cornell, textured, name, size, jitter, bounded, K=K1, breaks=()):
    """(image (H, W, 4), rays) of a flat case, computed once and never written again"""
    key = (name, size, jitter, bounded, K, tuple(breaks))
    if key not in _REF:
        mesh, _ = flat_variants(cr, cornell, textured)[name]
        scene = ao_ref.RefScene(mesh, cornell[1], *size)
        img, rays = ao_ref.render_ao(scene, RV[0], RV[1], K, radius_of(mesh, bounded), jitter=jitter, breaks=breaks)
        img.setflags(write=False)
        _REF[key] = (img, rays)
    return _REF[key]


# ---------------------------------------------------------------- C1 ----

def test_c1_the_entries_are_exported_and_refuse_null_scenes(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    for name in ("crt_render_ao", "crt_read_ao", "crt_ao_device", "crt_ao_points", "crt_ao_points_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    assert cr.AO_POINT_DT.itemsize == 32 and cr.AO_POINT_DT.names == ("p", "seed_x", "n", "seed_y")
    assert cr.AO_POINT_DT == ao_ref.AO_POINT_DT
    assert C.sizeof(_lib.crt_ao_params) == 32
    buf = np.zeros(8, f32)
    ptr = buf.ctypes.data_as(C.c_void_p)
    p = C.c_void_p()
    assert L.crt_render_ao(None, 0.0, 0.0, None, 1) == _lib.CRT_ERR_INVALID and b"null scene" in L.crt_last_error()
    assert L.crt_read_ao(None, ptr, 8) == _lib.CRT_ERR_INVALID
    assert L.crt_ao_device(None, C.byref(p)) == _lib.CRT_ERR_INVALID and not p.value
    assert L.crt_ao_points(None, ptr, 1, 0.0, 0.0, None, ptr) == _lib.CRT_ERR_INVALID and b"null scene" in L.crt_last_error()
    assert L.crt_ao_points_device(None, ptr, 1, 0.0, 0.0, None, ptr, 1) == _lib.CRT_ERR_INVALID and b"null scene" in L.crt_last_error()
    assert not buf.any()
    assert L.crt_abi_version() == 6
    for name in ("render_ao", "read_ao", "ao_device", "ao_points", "ao_points_device"):
        assert callable(getattr(cr.Scene, name))


# ---------------------------------------------------------------- C2: the sampler by its own properties ----

def test_c2_the_sampler_is_orthonormal_unit_length_and_cosine_distributed():
    """`bu`, `bv`, `nn` orthonormal to 4e-6 is read as: each of unit LENGTH to 4e-6 (as the directions' bound is stated) and pairwise dots
    within 4e-6 of 0.  A SQUARED length does not keep that bound: the basis turns the normal's own rounding error d = |nn|^2 - 1 (up to
    2.6e-7 here) into nn.x^2 a^2 d, 4.8e-6 for the normal (0.418, -0.084, -0.905) of this draw, whose length is off by 2.4e-6."""
    rng = np.random.default_rng(11)
    n = rng.normal(size=(64, 3))
    n = np.concatenate([n / np.linalg.norm(n, axis=1, keepdims=True), [[0, 0, -1], [0, 0, 1]]]).astype(f32)
    ok, nn, _, bu, bv = ao_ref.frame(np.zeros_like(n), n, ao_ref.OFFSET)
    assert ok.all()
    d = lambda a, b: (a.astype(np.float64) * b.astype(np.float64)).sum(-1)
    for a in (bu, bv, nn):                                                      # unit LENGTH to 4e-6, as the directions below
        assert np.abs(np.sqrt(d(a, a)) - 1).max() <= 4e-6
    for a, b in ((bu, bv), (bu, nn), (bv, nn)):
        assert np.abs(d(a, b)).max() <= 4e-6
    assert np.array_equal(bu[64], f32([0, -1, 0])) and np.array_equal(bv[64], f32([-1, 0, 0]))      # (0, 0, -1): the singular basis
    K, seeds = 256, 64
    m = n.shape[0]
    sx, sy = rng.uniform(0.5, 2000.0, m * seeds).astype(f32), rng.uniform(0.5, 2000.0, m * seeds).astype(f32)
    rep = lambda a: np.repeat(a, seeds, 0)
    sd = ao_ref.directions(rep(nn), rep(bu), rep(bv), sx, sy, K, f32(RV[0]) * f32(RV[1]))
    assert np.abs(np.sqrt(d(sd, sd)) - 1).max() <= 4e-6
    cos = d(sd, rep(nn)[:, None, :]).reshape(m, seeds * K).mean(1)
    # a cosine-weighted cosine has mean 2/3 and standard deviation sqrt(1/18)
    se = np.sqrt(1.0 / 18.0) / np.sqrt(K * seeds)
    print("C2: worst deviation of the mean cosine in standard errors:", np.abs(np.array(cos) - 2.0 / 3.0).max() / se)
    assert np.abs(np.array(cos) - 2.0 / 3.0).max() <= 4 * se


# ---------------------------------------------------------------- C3: the premise of the GPU checks ----

@pytest.mark.parametrize("name,size", CASES)
def test_c3_the_oracle_walk_and_the_brute_force_agree_on_every_ray(cr, ob, cornell, textured, name, size):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    orc = ob.Oracle(flat_data(cr, mesh, cam, "sbvh"), size[0], size[1], 1, camera=cam)
    for jitter in (0, 1):
        images = {}
        for bounded in (False, True):
            img, r = flat_ref(cr, cornell, textured, name, size, jitter, bounded)
            idx = np.nonzero(r["ok"])[0]
            rays = np.zeros(idx.size * K1, cr.RAY_DT)
            rays["o"], rays["d"], rays["tmax"] = np.repeat(r["o"][idx], K1, 0), r["sd"][idx].reshape(-1, 3), radius_of(mesh, bounded)
            hit = orc.trace(rays, ob.BVH8, ob.ANY, ob.TIE_LOWEST_ID, threads=THREADS)["tri"] >= 0
            disagree = int((hit != ~r["visible"][idx].reshape(-1)).sum())
            ao = img.reshape(-1, 4)[:, 3]
            counts = dict(miss=int((ao == -1).sum()), open=int((ao == 1).sum()), part=int(((ao > 0) & (ao < 1)).sum()), closed=int((ao == 0).sum()))
            print(f"C3 {name} {size} jitter {jitter} bounded {bounded}: rays {rays.shape[0]}, disagreements {disagree}, pixels {counts}")
            assert disagree == 0
            assert counts["miss"] > 0 and counts["open"] > 0 and counts["part"] > 0, counts
            images[bounded] = img
        assert (words(images[False]) != words(images[True])).any()


# ---------------------------------------------------------------- C4: the analytic ends ----

def closed_box(cam):
    V = np.array([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)], f32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    tri = np.zeros((12, 12), np.int32)
    for q, (a, b, c, d) in enumerate(quads):
        tri[2 * q, :3], tri[2 * q + 1, :3] = (a, b, c), (a, c, d)
    tri[:, 4:8] = (0, 1, 0, 0)
    mats = np.zeros((1, 16), f32)
    mats[0, 7] = mats[0, 12] = -1
    mesh = types.SimpleNamespace(vertices=V, normals=np.zeros((0, 3), f32), texcoords=np.zeros((0, 2), f32), triangles=tri, materials=mats,
                                 lights=np.zeros((0, 18), f32))
    return ao_ref.RefScene(mesh, cam, 8, 8)


def test_c4_inside_a_closed_box_everything_or_nothing_is_occluded(cornell):
    scene = closed_box(cornell[1])
    rng = np.random.default_rng(3)
    pts = np.zeros(64, ao_ref.AO_POINT_DT)
    pts["p"] = rng.uniform(-0.5, 0.5, (64, 3))
    pts["n"] = rng.normal(size=(64, 3))
    pts["seed_x"], pts["seed_y"] = rng.uniform(0.5, 500, 64), rng.uniform(0.5, 500, 64)
    closed, _ = ao_ref.ao_points(scene, pts, 16, *RV, radius=f32(4.0))            # >= the diagonal 2 sqrt(3)
    assert (closed == f32([0, 0, 0, 0])).all()
    opened, r = ao_ref.ao_points(scene, pts, 16, *RV, radius=f32(0.45))           # below the 0.5 to the nearest wall (less the offset)
    assert (opened[:, 3] == 1).all()
    b = np.zeros((64, 3), f32)
    for k in range(16):
        b = (b + r["sd"][:, k]).astype(f32)
    assert np.array_equal(words(opened)[:, :3], b.view(np.uint32))


# ---------------------------------------------------------------- C5: the mistakes the scenes must notice ----

@pytest.fixture(scope="module")
def yard_scene(cr, textured):
    return yard(cr, textured[0].albedo_textures)


_YARD = {}


def yard_ref(s, options, key, K=K1, radius=ao_ref.UNBOUNDED, breaks=(), rv=RV):
    k = (key, K, float(radius), tuple(breaks), rv)
    if k not in _YARD:
        scene = ref_scene(s, options)
        img, rays = ao_ref.render_ao(scene, rv[0], rv[1], K, radius, jitter=1, breaks=breaks)
        img.setflags(write=False)
        _YARD[k] = (img, rays)
    return _YARD[k]


@pytest.mark.parametrize("brk", ao_ref.BREAKS)
def test_c5_a_mistake_in_the_reference_changes_words(cr, cornell, textured, yard_scene, brk):
    want = flat_ref(cr, cornell, textured, "cornell", SMALL, 1, False)[0]
    got = flat_ref(cr, cornell, textured, "cornell", SMALL, 1, False, breaks=(brk,))[0]
    diff = int((words(got) != words(want)).sum())
    diff_y = int((words(yard_ref(yard_scene, None, "Y", breaks=(brk,))[0]) != words(yard_ref(yard_scene, None, "Y")[0])).sum())
    print(f"C5 {brk}: differing words on cornell {diff}, on the yard {diff_y}")
    assert diff + diff_y > 0


# ---------------------------------------------------------------- G1: flat views ----

@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sbvh", "sah"])
@pytest.mark.parametrize("name,size", CASES)
def test_g1_flat_views_bit_for_bit(cr, cornell, textured, name, size, builder):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    sc = flat_scene(cr, mesh, cornell[1], builder, *size)
    for jitter in (0, 1):
        sc.set_option("jitter", jitter)
        for bounded in (False, True):
            want = flat_ref(cr, cornell, textured, name, size, jitter, bounded)[0]
            sc.render_ao(*RV, samples=K1, radius=radius_of(mesh, bounded))
            assert_words(sc.read_ao(), want, (name, size, builder, jitter, bounded))
    assert sc.frame_stats()["stack_overflows"] == 0
    sc.close()


# ---------------------------------------------------------------- G2: the definition itself ----

def device_array(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).cuda()


@pytest.mark.gpu
@pytest.mark.parametrize("bounded", [False, True])
def test_g2_the_rays_through_crt_trace_device_fold_to_the_same_bytes(cr, cornell, textured, bounded):
    import torch
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    _, r = flat_ref(cr, cornell, textured, "textured", LARGE, 1, bounded)
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", *LARGE)
    sc.render_ao(*RV, samples=K1, radius=radius_of(mesh, bounded))
    got = sc.read_ao()
    n = r["ok"].shape[0]
    rays = np.zeros(n * K1, cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = np.repeat(r["o"], K1, 0), r["sd"].reshape(-1, 3), radius_of(mesh, bounded)
    d_rays, d_hits = device_array(rays), torch.zeros(n * K1 * 16, dtype=torch.uint8, device="cuda")
    sc.trace_device(d_rays.data_ptr(), n * K1, d_hits.data_ptr(), mode=cr.CRT_TRACE_ANY)
    hits = d_hits.cpu().numpy().view(cr.HIT_DT)
    visible = (hits["tri"] < 0).reshape(n, K1) & r["ok"][:, None]
    assert_words(got, ao_ref.fold(r["ok"], r["sd"], visible), ("trace_device", bounded))
    sc.close()


# ---------------------------------------------------------------- G3: points mode ----

@pytest.mark.gpu
def test_g3_points_mode_gives_the_views_bytes(cr, cornell, textured):
    import torch
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    want, r = flat_ref(cr, cornell, textured, "textured", LARGE, 1, False)
    want = want.reshape(-1, 4)
    pts = r["points"]
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", *LARGE)
    got = sc.ao_points(pts, *RV, samples=K1)                                     # the whole view, miss pixels included
    assert_words(got, want, "host form, the view")
    d_pts, d_out = device_array(pts), torch.zeros(pts.shape[0] * 16, dtype=torch.uint8, device="cuda")
    sc.ao_points_device(d_pts.data_ptr(), pts.shape[0], d_out.data_ptr(), *RV, samples=K1)
    assert_words(d_out.cpu().numpy().view(f32), want, "device form, the view")
    hit = np.nonzero(r["ok"])[0]
    for n in (1, 63, 64, 65, 515):                                               # 515 x 8 entries: beyond 4096, and several pools of 256
        idx = hit[7:7 + n]
        assert_words(sc.ao_points(pts[idx], *RV, samples=K1), want[idx], ("n", n))
    # n = 0 succeeds and writes nothing
    assert sc.ao_points(pts[:0], *RV, samples=K1).shape == (0, 4)
    sc.ao_points_device(0, 0, 0, *RV, samples=K1)
    # points without rays between points with: (0, 0, 0, -1), the neighbours right
    idx = hit[100:107]
    odd = pts[idx].copy()
    odd["n"][1] = 0
    odd["n"][3] = (np.nan, 1, 0)
    odd["p"][5] = (np.inf, 0, 0)
    res = sc.ao_points(odd, *RV, samples=K1)
    expect = want[idx].copy()
    expect[[1, 3, 5]] = (0, 0, 0, -1)
    assert_words(res, expect, "points without rays")
    # n = (0, 0, -1) takes the singular basis; normals of other lengths and directions against the reference
    scene = ao_ref.RefScene(mesh, cornell[1], *LARGE)
    mine = pts[hit[200:264]].copy()
    mine["n"][:8] = (0, 0, -1)
    mine["n"][8:16] = (0, 0, -3.5)
    mine["n"][16:] = np.random.default_rng(5).normal(size=(48, 3)) * 2.0
    ref, _ = ao_ref.ao_points(scene, mine, 16, *RVS[1], radius=f32(150.0), offset=f32(0.01))
    assert_words(sc.ao_points(mine, *RVS[1], samples=16, radius=150.0, offset=0.01), ref, "free points")
    sc.close()


# ---------------------------------------------------------------- G4: K at the word boundaries ----

@pytest.mark.gpu
@pytest.mark.parametrize("K", [1, 31, 32, 33, 256])
def test_g4_sample_counts_at_the_word_boundaries(cr, cornell, textured, K):
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    want = flat_ref(cr, cornell, textured, "cornell", SMALL, 1, False, K=K)[0]
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", *SMALL)
    sc.render_ao(*RV, samples=K)
    assert_words(sc.read_ao(), want, K)
    sc.close()


# ---------------------------------------------------------------- G5: instanced scenes ----

@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_g5_identity_instances_give_the_flat_scenes_bytes(cr, cornell, textured, builder):
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    for bounded in (False, True):
        want = flat_ref(cr, cornell, textured, "textured", SMALL, 1, bounded)[0]
        inst, sc, _ = identity_scene(cr, mesh, parts, builder, *SMALL)
        sc.update(cornell[1])
        sc.render_ao(*RV, samples=K1, radius=radius_of(mesh, bounded))
        assert_words(sc.read_ao(), want, (builder, bounded))
        sc.close()
        inst.close()


def fold_of_the_handles_trace(cr, inst, r, K, radius, ray_mask):
    """the reference's rays through crt_instances_trace_device(ANY [| INSTANCE_MASK]), the mask in the rays' pad words, folded in numpy"""
    import torch
    n = r["ok"].shape[0]
    rays = np.zeros(n * K, cr.RAY_DT)
    rays["o"], rays["d"], rays["tmax"] = np.repeat(r["o"], K, 0), r["sd"].reshape(-1, 3), radius
    mode = cr.CRT_TRACE_ANY
    if ray_mask is not None:
        rays["pad"] = ray_mask
        mode |= cr.CRT_TRACE_INSTANCE_MASK
    d_rays, d_hits = device_array(rays), torch.zeros(n * K * 16, dtype=torch.uint8, device="cuda")
    inst.trace_device(d_rays.data_ptr(), n * K, d_hits.data_ptr(), mode=mode)
    hits = d_hits.cpu().numpy().view(cr.HIT_DT)
    return ao_ref.fold(r["ok"], r["sd"], (hits["tri"] < 0).reshape(n, K) & r["ok"][:, None])


@pytest.mark.gpu
def test_g5_general_transforms_across_a_refit_and_a_set(cr, textured, yard_scene):
    y = yard_scene
    moved = yard(cr, textured[0].albedo_textures, moved=True)
    inst, sc = open_scene(cr, y, 1)
    radius = f32(2.5)
    for bounded in (False, True):
        rad = radius if bounded else ao_ref.UNBOUNDED
        want, r = yard_ref(y, None, "Y", radius=rad)
        sc.render_ao(*RV, samples=K1, radius=rad)
        got = sc.read_ao()
        assert_words(got, want, ("created", bounded))
        assert_words(got, fold_of_the_handles_trace(cr, inst, r, K1, rad, None), ("created, the handle's trace", bounded))
    ao = want.reshape(-1, 4)[:, 3]
    assert (ao == -1).any() and (ao == 1).any() and ((ao > 0) & (ao < 1)).any()
    assert (words(yard_ref(y, None, "Y")[0]) != words(want)).any()               # the radius matters
    rec = cr.instances_array(moved.M, moved.mesh_of, masks=moved.masks, material_offsets=moved.offsets)
    inst.refit(rec)                                                               # seen by the next call, no crt_reset
    want2 = yard_ref(moved, None, "Y'")[0]
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), want2, "refitted")
    assert (words(want2) != words(yard_ref(y, None, "Y")[0])).any()
    inst.set(cr.instances_array(y.M, y.mesh_of, masks=y.masks, material_offsets=y.offsets))
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), yard_ref(y, None, "Y")[0], "set back")
    sc.close()
    inst.close()


@pytest.mark.gpu
def test_g5_masks_hide_occluders_and_points(cr, yard_scene):
    y = yard_scene
    plain, r_plain = yard_ref(y, None, "Y")
    masked, r = yard_ref(y, MASKS_ON, "Y masked")
    shadow_open, r_open = yard_ref(y, {**MASKS_ON, "mask_shadow": 0xff}, "Y masked, shadow rays see all")
    point_words = lambda rr: rr["points"].view(np.uint32).reshape(-1, 8)
    moved = (point_words(r_plain) != point_words(r)).any(1)
    print("G5 masks: pixels whose point mask_primary changes:", int(moved.sum()))
    assert moved.sum() >= 1                                                       # mask_primary changes which surface a pixel's point lies on
    assert np.array_equal(point_words(r), point_words(r_open))                    # mask_shadow changes no point ...
    assert (words(masked) != words(shadow_open)).any()                            # ... and hides an occluder
    inst, sc = open_scene(cr, y, 1, options=MASKS_ON)
    sc.render_ao(*RV, samples=K1)
    got = sc.read_ao()
    assert_words(got, masked, "masked")
    assert_words(got, fold_of_the_handles_trace(cr, inst, r, K1, ao_ref.UNBOUNDED, MASKS_ON["mask_shadow"]), "masked, the handle's trace")
    sc.set_option("mask_shadow", 0xff)
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), shadow_open, "mask_shadow 255")
    sc.set_option("instance_masks", 0)
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), plain, "option back to 0")
    sc.close()
    inst.close()


# ---------------------------------------------------------------- G6: nothing else moves ----

QUEUE_ORDER_FIELDS = ("wave_steps_closest_nodes", "wave_steps_closest_tris", "wave_steps_any_nodes", "wave_steps_any_tris")      # see test_aov.py


def frames_state(sc, depth):
    st = sc.frame_stats()
    if depth > 1:
        st = {k: v for k, v in st.items() if k not in QUEUE_ORDER_FIELDS}
    return sc.read_sum(), st, sc.frame_count


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g6_a_call_between_frames_changes_nothing_else(cr, cornell, textured, kind, depth):
    mesh, parts = flat_variants(cr, cornell, textured)["tess8_mat"]
    cam = cornell[1]
    W, H = LARGE

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
    plain.render_ao(*RVS[3], samples=K1)
    want_ao = plain.read_ao()
    close_plain()
    sc, closer = make()
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    stats3 = sc.frame_stats()
    sc.render_aov(*RVS[2])
    aov = read_all(cr, sc)
    sc.render_ao(*RVS[3], samples=K1)
    assert_words(sc.read_ao(), want_ao, "between frames")
    assert sc.frame_stats() == stats3
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(np.ascontiguousarray(after[n]).view(np.uint8), np.ascontiguousarray(aov[n]).view(np.uint8)), n
    for rv in RVS[3:5]:
        sc.render_frame(*rv)
    got_sum, got_stats, got_count = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats and got_count == want_count
    closer()
    # enqueued without a host wait behind asynchronous frames, a frame behind it
    sc, closer = make()
    sc.render_frames(RVS[:3], sync=False)
    sc.render_ao(*RVS[3], samples=K1, sync=False)
    for rv in RVS[3:5]:
        sc.render_frame(*rv, sync=False)
    sc.sync()
    assert_words(sc.read_ao(), want_ao, "async")
    got_sum, got_stats, _ = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32)) and got_stats == want_stats
    closer()


@pytest.mark.gpu
def test_g6_a_lens_and_an_environment_change_no_byte(cr, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    want = flat_ref(cr, cornell, textured, "textured", SMALL, 1, False)[0]
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", *SMALL)
    sc.update(lens_camera(cr, cornell[1], 0.05, 3.0))
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), want, "lens")
    sc.set_environment(cr.constant_environment((0.5, 0.7, 1.0)))
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), want, "lens and environment")
    sc.close()


# ---------------------------------------------------------------- G7: refusals and lifetime ----

@pytest.mark.gpu
def test_g7_refusals_name_the_field_and_leave_the_image(cr, cornell, textured):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    W, H = SMALL
    want = flat_ref(cr, cornell, textured, "textured", SMALL, 1, False)[0]
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", W, H)
    L = _lib.lib()

    def refused(call, word):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == CRT_ERR_INVALID and word in str(e.value), (word, e.value)

    refused(lambda: sc.read_ao(), "no crt_render_ao")                             # a read before any render
    refused(lambda: sc.ao_device(), "no crt_render_ao")
    sc.render_frame(*RV)
    sum_before = sc.read_sum()
    sc.render_ao(*RV, samples=K1)
    assert_words(sc.read_ao(), want, "first")
    pts = np.zeros(4, cr.AO_POINT_DT)
    pts["n"] = (0, 1, 0)
    out = np.full((4, 4), 7, f32)

    def params(**kw):
        p = _lib.crt_ao_params()
        p.samples, p.flags, p.radius, p.offset = 16, 0, 1e9, 2e-4
        for k, v in kw.items():
            if k == "reserved":
                p.reserved[v] = 1
            else:
                setattr(p, k, v)
        return p

    def entries(p):
        ptr, optr = pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
        return [lambda: _lib.check(L.crt_render_ao(sc._h, 0.3, 0.8, C.byref(p), 1)),
                lambda: _lib.check(L.crt_ao_points(sc._h, ptr, 4, 0.3, 0.8, C.byref(p), optr)),
                lambda: _lib.check(L.crt_ao_points_device(sc._h, ptr, 4, 0.3, 0.8, C.byref(p), optr, 1))]

    bad = [(dict(samples=0), "samples"), (dict(samples=257), "samples"), (dict(radius=0.0), "radius"), (dict(radius=-1.0), "radius"),
           (dict(radius=float("inf")), "radius"), (dict(radius=float("nan")), "radius"), (dict(offset=-1e-6), "offset"),
           (dict(offset=float("nan")), "offset"), (dict(offset=float("inf")), "offset"), (dict(flags=1), "flags"), (dict(reserved=0), "reserved"),
           (dict(reserved=3), "reserved")]
    for kw, word in bad:
        for call in entries(params(**kw)):
            refused(call, word)
    ptr, optr = pts.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    refused(lambda: _lib.check(L.crt_ao_points(sc._h, None, 4, 0.3, 0.8, None, optr)), "null")
    refused(lambda: _lib.check(L.crt_ao_points(sc._h, ptr, 4, 0.3, 0.8, None, None)), "null")
    refused(lambda: _lib.check(L.crt_ao_points_device(sc._h, None, 4, 0.3, 0.8, None, optr, 1)), "null")
    refused(lambda: _lib.check(L.crt_ao_points_device(sc._h, ptr, 4, 0.3, 0.8, None, None, 1)), "null")
    p256 = params(samples=256)
    refused(lambda: _lib.check(L.crt_ao_points_device(sc._h, ptr, 1 << 24, 0.3, 0.8, C.byref(p256), optr, 1)), "2^32")      # n * K = 2^32
    refused(lambda: _lib.check(L.crt_ao_points(sc._h, ptr, 1 << 24, 0.3, 0.8, C.byref(p256), optr)), "2^32")
    buf = np.zeros(W * H * 4, f32)
    refused(lambda: _lib.check(L.crt_read_ao(sc._h, buf.ctypes.data_as(C.c_void_p), W * H * 4 - 4)), "n_floats")
    refused(lambda: _lib.check(L.crt_read_ao(sc._h, buf.ctypes.data_as(C.c_void_p), W * H * 3)), "n_floats")
    sc.set_option("accel", 1)
    for call in entries(params()):
        refused(call, "accel")
    sc.set_option("accel", 0)
    assert (out == 7).all() and not buf.any()
    assert_words(sc.read_ao(), want, "after the refusals")
    assert np.array_equal(sc.read_sum().view(np.uint32), sum_before.view(np.uint32))
    p = sc.ao_device()
    assert p and np.array_equal(device_bytes_at(p, W * H * 16), np.ascontiguousarray(want).view(np.uint8).reshape(-1))
    sc.set_devices([0, 0])                                     # two logical devices behind the handle
    for call in entries(params()):
        refused(call, "one device")
    sc.set_devices([0])
    assert_words(sc.read_ao(), want, "after set_devices")
    sc.close()
    # a shard of a frame; a frame too large for 32-bit entry indices
    sc = flat_scene(cr, mesh, cornell[1], "sbvh", W, H)
    sc.set_shard(1, 2, 16)
    for call in entries(params()):
        refused(call, "crt_set_shard")
    sc.close()
    big = flat_scene(cr, mesh, cornell[1], "sbvh", 8192, 4096)
    refused(lambda: big.render_ao(*RV, samples=128), "2^32")                      # 2^25 pixels x 2^7
    big.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g7_ten_calls_hold_the_memory_of_the_first(cr, cornell, textured, kind):
    import torch
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    if kind == "flat":
        sc, inst = flat_scene(cr, mesh, cornell[1], "sbvh", *LARGE), None
    else:
        inst, sc, _ = identity_scene(cr, mesh, parts, "sah", *LARGE)
        sc.update(cornell[1])
    used = []
    for k in range(10):
        sc.render_ao(*RVS[k % 8], samples=K1)
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
    print("device bytes in use after each render_ao:", used)
    assert all(u == used[0] for u in used), used
    sc.close()
    if inst is not None:
        inst.close()


@pytest.mark.gpu
def test_g7_after_rebuild_vertices_the_image_shows_the_new_positions(cr, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["cornell"]
    cam = cornell[1]
    rng = np.random.default_rng(5)
    moved = cr.Mesh((mesh.vertices + rng.uniform(-0.15, 0.15, mesh.vertices.shape)).astype(f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials,
                    mesh.lights, mesh.vertex_min)
    sc = flat_scene(cr, mesh, cam, "sah", *SMALL)
    sc.render_ao(*RV, samples=K1)
    before = flat_ref(cr, cornell, textured, "cornell", SMALL, 1, False)[0]
    assert_words(sc.read_ao(), before, "built")
    sc.rebuild_vertices(moved.vertices)
    sc.render_ao(*RV, samples=K1)
    want = ao_ref.render_ao(ao_ref.RefScene(moved, cam, *SMALL), RV[0], RV[1], K1)[0]
    assert_words(sc.read_ao(), want, "rebuilt")
    assert (words(want) != words(before)).any()
    sc.close()
