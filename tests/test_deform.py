"""Deformation on the device (include/crt.h crt_deformer_create .. crt_deform_host).  crt_deform_host and the kernel are
held to tests/deform_ref.py, the header's definition in float32 numpy, byte for byte; a scene deformed by crt_deform_scene is held to a
second scene given the reference's arrays through crt_update_vertices / crt_rebuild_vertices: accel bytes, walks and frames."""
import ctypes as C

import numpy as np
import pytest

from conftest import seeded_rays
from deform_ref import deform_ref

f32 = np.float32
RX1, RY1 = 0.6591631174087524, 0.9108020067214966
IDENTITY = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], f32)
SIZES = [1, 63, 64, 65, 257, 4099]
BONES = [1, 2, 7, 300]


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _weights(rng, n):
    """four weights per element: some rows sum to one, some do not, some are negative, and every position after the first is an exact
    zero somewhere (alone and together with the others); the first is zero somewhere too"""
    w = rng.random((n, 4)).astype(f32)
    w = (w / w.sum(1, keepdims=True)).astype(f32)
    kind = np.arange(n) % 11
    for k in (1, 2, 3):
        w[kind == k, k] = 0.0
    w[kind == 4, 1:] = 0.0
    w[kind == 5, 2:] = 0.0
    w[kind == 6, 0] = 0.0
    w[kind == 7] *= f32(-1.5)
    w[kind == 8, 2] = f32(-0.25)
    w[kind == 9] *= f32(3.0)
    w[kind == 4, 1] = -0.0                # a negative zero is a zero: skipped
    return w


def make_case(seed, nv, n_bones, n_targets=5):
    """A seeded deformer input: nv vertices, nv + 3 normals, n_bones random affine bones; vertex 0 is listed by all five targets,
    vertex 1 by target 2 alone, vertex 2 by none, the others at random; normals 0 and 1 are so short that l2 falls below 0x1p-126f,
    normal 2 so long that l2 overflows."""
    rng = np.random.default_rng(seed)
    nn = nv + 3
    c = {"rest_vertices": rng.uniform(-2, 2, (nv, 3)).astype(f32), "vertex_bones": rng.integers(0, n_bones, (nv, 4)).astype(np.uint16),
         "vertex_weights": _weights(rng, nv)}
    n = rng.normal(size=(nn, 3))
    n = (n / np.linalg.norm(n, axis=1, keepdims=True)).astype(f32)
    n[0] *= f32(1e-30)
    n[1] *= f32(1e-21)
    n[2] *= f32(1e25)
    c.update(rest_normals=n, normal_bones=rng.integers(0, n_bones, (nn, 4)).astype(np.uint16), normal_weights=_weights(rng, nn))
    c["vertex_bones"][0, 0] = n_bones - 1
    targets = []
    for t in range(n_targets):
        on = rng.random(nv) < 0.3
        on[0] = True
        if nv > 1:
            on[1] = t == 2
        if nv > 2:
            on[2] = False
        idx = np.nonzero(on)[0].astype(np.uint32)
        targets.append((idx, rng.normal(scale=0.2, size=(idx.shape[0], 3)).astype(f32)))
    c["morph_targets"] = targets
    bones = rng.normal(size=(n_bones, 3, 4)).astype(f32)
    mw = rng.uniform(-1, 1, n_targets).astype(f32)
    return c, bones, mw


def _listed(case, nv):
    count = np.zeros(nv, np.int64)
    for idx, _ in case["morph_targets"]:
        count[idx] += 1
    return count


def _equal(got, want):
    (gv, gn), (wv, wn) = got, want
    assert np.array_equal(_bits(gv), _bits(wv)), np.nonzero((gv.view(np.uint32) != wv.view(np.uint32)).any(1))[0][:8]
    assert (gn is None) == (wn is None)
    if wn is not None:
        assert np.array_equal(_bits(gn), _bits(wn)), np.nonzero((gn.view(np.uint32) != wn.view(np.uint32)).any(1))[0][:8]


# ------------------------------------------------------------------------------------------------------------ host (no GPU) --

def test_entry_points_are_exported_and_bound(cr):
    from caitlynrenderer_amd import _lib
    for name in ("crt_deformer_create", "crt_deformer_destroy", "crt_deformer_pose", "crt_deformer_sync", "crt_deformer_vertices_device",
                 "crt_deformer_normals_device", "crt_deformer_read", "crt_deformer_last_ms", "crt_deform_scene", "crt_deform_host"):
        assert name in _lib.SYMBOLS and hasattr(_lib.lib(), name)
    assert hasattr(cr.Scene, "deform") and hasattr(cr, "Deformer") and hasattr(cr, "deform_host") and hasattr(cr, "normal_influences")
    assert _lib.lib().crt_abi_version() == 6


@pytest.mark.parametrize("n_bones", BONES)
@pytest.mark.parametrize("nv", SIZES)
def test_host_equals_the_reference(cr, nv, n_bones):
    case, bones, mw = make_case(1000 * nv + n_bones, nv, n_bones)
    if nv > 2:
        assert set(_listed(case, nv)[:3]) == {5, 1, 0}
    for weights in (mw, None, np.zeros_like(mw)):
        want = deform_ref(bones, morph_weights=weights, **case)
        _equal(cr.deform_host(bones, morph_weights=weights, **case), want)
    l2 = (want[1].astype(np.float64) ** 2).sum(1)
    assert not np.isfinite(want[1][2]).all() or l2[2] > 2.0      # normal 2 overflowed: left as q, not a unit vector
    assert l2[0] < 1e-30                                         # normal 0 underflowed: left as q


def test_host_without_normals_and_without_targets(cr):
    case, bones, _ = make_case(7, 65, 7)
    plain = {k: case[k] for k in ("rest_vertices", "vertex_bones", "vertex_weights")}
    got = cr.deform_host(bones, n_bones=7, **plain)
    assert got[1] is None
    _equal(got, deform_ref(bones, **plain))


def _rig(n, bone_of=0):
    return np.full((n, 4), bone_of, np.uint16), np.tile(np.array([1, 0, 0, 0], f32), (n, 1))


def test_identity_bones_give_the_rest_pose(cr):
    case, _, _ = make_case(3, 257, 4)
    b, w = _rig(257)
    nb, nw = _rig(260)
    n = case["rest_normals"][3:].copy()                     # unit normals
    n[:2] = [[0, 0, 1], [-1, 0, 0]]
    v, nn = cr.deform_host(np.tile(IDENTITY, (4, 1, 1)), case["rest_vertices"], b, w, n, nb[:257], nw[:257])
    assert (v == case["rest_vertices"]).all()
    assert (nn[:2] == n[:2]).all() and np.abs(nn - n).max() <= 2 ** -23      # axis normals exactly; the others renormalised within an ulp


def test_a_translation_moves_every_vertex_by_exactly_it(cr):
    rng = np.random.default_rng(5)
    rest = (rng.integers(-4096, 4096, (300, 3)) / 64.0).astype(f32)       # multiples of 1/64: the sums below are exact
    n = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0], [0, -1, 0]], f32)
    T = IDENTITY.copy()
    T[:, 3] = [2.5, -0.125, 1024.0]
    b, w = _rig(300)
    nb, nw = _rig(4)
    v, nn = cr.deform_host(T[None], rest, b, w, n, nb, nw)
    assert (v == rest + T[:, 3]).all() and (nn == n).all()


def test_two_half_weight_bones_one_translated(cr):
    rng = np.random.default_rng(6)
    rest = (rng.integers(-4096, 4096, (100, 3)) / 64.0).astype(f32)
    T = IDENTITY.copy()
    T[0, 3] = 2.0
    b = np.tile(np.array([0, 1, 0, 0], np.uint16), (100, 1))
    w = np.tile(np.array([0.5, 0.5, 0, 0], f32), (100, 1))
    v, _ = cr.deform_host(np.stack([IDENTITY, T]), rest, b, w)
    assert (v == rest + np.array([1, 0, 0], f32)).all()


def _refusals():
    """name -> a function that spoils (case, bones, morph_weights) in place"""
    def put(key, index, value):
        def f(c, bones, mw):
            c[key][index] = value
        return f

    def target(t, fn):
        def f(c, bones, mw):
            idx, d = c["morph_targets"][t]
            c["morph_targets"][t] = fn(idx.copy(), d.copy())
        return f

    def swap(idx, d):
        idx[[0, 1]] = idx[[1, 0]]
        return idx, d

    def repeat(idx, d):
        idx[1] = idx[0]
        return idx, d

    def out_of_range(idx, d):
        idx[-1] = 65
        return idx, d

    def nan_delta(idx, d):
        d[0, 1] = np.nan
        return idx, d

    def bone(i, value):
        def f(c, bones, mw):
            bones[i, 1, 2] = value
        return f

    def weight(c, bones, mw):
        mw[3] = np.inf
    return {"rest nan": put("rest_vertices", (3, 1), np.nan), "rest inf": put("rest_vertices", (64, 0), -np.inf),
            "rest huge": put("rest_vertices", (0, 2), f32(3e18)), "weight nan": put("vertex_weights", (5, 3), np.nan),
            "normal inf": put("rest_normals", (2, 0), np.inf), "normal weight inf": put("normal_weights", (67, 0), np.inf),
            "vertex bone": put("vertex_bones", (9, 2), 7), "normal bone": put("normal_bones", (0, 0), 65535),
            "target order": target(1, swap), "target repeat": target(4, repeat), "target vertex": target(0, out_of_range),
            "delta nan": target(2, nan_delta), "bone nan": bone(0, np.nan), "bone inf": bone(6, np.inf), "morph weight inf": weight}


@pytest.mark.parametrize("bad", sorted(_refusals()))
def test_host_refusals_leave_the_outputs_untouched(cr, bad):
    from caitlynrenderer_amd import _lib
    case, bones, mw = make_case(11, 65, 7)
    case = {k: (list(v) if k == "morph_targets" else v.copy()) for k, v in case.items()}
    _refusals()[bad](case, bones, mw)
    from caitlynrenderer_amd.deform import _Desc
    d = _Desc(n_bones=7, **case)
    out_v, out_n = np.full((65, 3), 7.5, f32), np.full((68, 3), -3.25, f32)
    rc = _lib.lib().crt_deform_host(C.byref(d.c), bones.ctypes.data, mw.ctypes.data, out_v.ctypes.data, out_n.ctypes.data)
    assert rc == _lib.CRT_ERR_INVALID and _lib.lib().crt_last_error().startswith(b"crt_deform_host: ")
    assert (out_v == 7.5).all() and (out_n == -3.25).all()


@pytest.mark.parametrize("bad", ["abi", "no vertices", "2^31 vertices", "2^31 normals", "no bones", "65537 bones", "65536 targets", "null weights",
                                 "normals without influences", "influences without normals", "first not 0", "first descends", "null bones",
                                 "null desc", "null out"])
def test_host_refuses_an_inconsistent_desc(cr, bad):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd.deform import _Desc
    case, bones, mw = make_case(12, 65, 7)
    d = _Desc(n_bones=7, **case)
    first = d.first.copy()
    args = [C.byref(d.c), bones.ctypes.data, mw.ctypes.data, None, None]
    out_v, out_n = np.full((65, 3), 7.5, f32), np.full((68, 3), -3.25, f32)
    args[3], args[4] = out_v.ctypes.data, out_n.ctypes.data
    if bad == "abi":
        d.c.abi_version = 5
    elif bad == "no vertices":
        d.c.n_vertices = 0
    elif bad == "2^31 vertices":
        d.c.n_vertices = 2 ** 31
    elif bad == "2^31 normals":
        d.c.n_normals = 2 ** 31
    elif bad == "no bones":
        d.c.n_bones = 0
    elif bad == "65537 bones":
        d.c.n_bones = 65537
    elif bad == "65536 targets":
        d.c.n_targets = 65536
    elif bad == "null weights":
        d.c.vertex_weights = None
    elif bad == "normals without influences":
        d.c.normal_bones = None
    elif bad == "influences without normals":
        d.c.n_normals, d.c.rest_normals = 0, None
    elif bad == "first not 0":
        first[0] = 1
        d.c.target_first = first.ctypes.data
    elif bad == "first descends":
        first[2] = first[1] - 1
        d.c.target_first = first.ctypes.data
    elif bad == "null bones":
        args[1] = None
    elif bad == "null desc":
        args[0] = None
    elif bad == "null out":
        args[3] = None
    assert _lib.lib().crt_deform_host(*args) == _lib.CRT_ERR_INVALID
    assert (out_v == 7.5).all() and (out_n == -3.25).all()


def test_create_checks_the_desc_before_the_device(cr):
    """A bad desc is CRT_ERR_INVALID with or without a GPU; a good one without a GPU is CRT_ERR_NO_DEVICE."""
    from caitlynrenderer_amd import _lib
    case, _, _ = make_case(13, 65, 7)
    bad = dict(case, vertex_bones=np.full((65, 4), 7, np.uint16))
    with pytest.raises(cr.CrtError) as e:
        cr.Deformer(n_bones=7, **bad)
    assert e.value.code == _lib.CRT_ERR_INVALID
    if _lib.lib().crt_device_count() <= 0:
        with pytest.raises(cr.CrtError) as e:
            cr.Deformer(n_bones=7, **case)
        assert e.value.code == _lib.CRT_ERR_NO_DEVICE
    for fn, args in (("crt_deformer_pose", (None, None, None, 1)), ("crt_deformer_sync", (None,)), ("crt_deformer_read", (None, None, 0, None, 0)),
                     ("crt_deform_scene", (None, None, None, None, 0, 1))):
        assert getattr(_lib.lib(), fn)(*args) == _lib.CRT_ERR_INVALID
    assert _lib.lib().crt_deformer_destroy(None) == _lib.CRT_OK


def test_normal_influences_on_a_hand_made_mesh(cr):
    """Four vertices, five normals; normal 1 is shared by corners of two triangles (its first use is triangle 0, corner 1: vertex 1),
    normal 3 is first used by triangle 1, corner 0 (vertex 3) although triangle 1, corner 2 uses it again with vertex 0; normal 4 is
    unused; triangle 2 carries no corner normals (vn.w == 0) and counts for nothing."""
    t = np.zeros((3, 12), np.int32)
    t[0, 0:3], t[0, 4:8] = (0, 1, 2), (0, 1, 2, 1)
    t[1, 0:3], t[1, 4:8] = (3, 2, 0), (3, 1, 3, 1)
    t[2, 0:3], t[2, 4:8] = (1, 2, 3), (4, 4, 4, 0)
    vb = np.arange(16, dtype=np.uint16).reshape(4, 4)
    vw = (np.arange(16, dtype=f32).reshape(4, 4) + 1) / 8
    nb, nw = cr.normal_influences(t, vb, vw, 5)
    assert nb.dtype == np.uint16 and nw.dtype == f32 and nb.shape == (5, 4) and nw.shape == (5, 4)
    for normal, vertex in ((0, 0), (1, 1), (2, 2), (3, 3)):
        assert (nb[normal] == vb[vertex]).all() and (nw[normal] == vw[vertex]).all()
    assert (nb[4] == 0).all() and (nw[4] == [1, 0, 0, 0]).all()


# ------------------------------------------------------------------------------------------------------------------ GPU --

# both ways the kernel reads the palette, held to the same bits: a workgroup's LDS copy up to 256 bones, the vector cache above and on request
@pytest.fixture(params=["auto", "global"])
def palette(request, monkeypatch):
    if request.param == "global":
        monkeypatch.setenv("CRT_DEFORM_PALETTE", "global")
    else:
        monkeypatch.delenv("CRT_DEFORM_PALETTE", raising=False)
    return request.param


@pytest.mark.gpu
@pytest.mark.parametrize("n_bones", BONES + [256, 257])       # 256 / 257: either side of the LDS palette limit
def test_pose_equals_the_reference(cr, palette, n_bones):
    """every size of the host test (the grid's tail: 1, 63 .. 65, 257, 4099 over tiles of 256) with every bone count, two poses on one handle"""
    for nv in SIZES:
        case, bones, mw = make_case(1000 * nv + n_bones, nv, n_bones)
        d = cr.Deformer(n_bones=n_bones, **case)
        d.pose(bones, mw)
        _equal(d.read(), deform_ref(bones, morph_weights=mw, **case))
        bones2 = (bones * f32(0.5) + f32(0.25)).astype(f32)
        d.pose(bones2, None, sync=False)
        _equal(d.read(), deform_ref(bones2, **case))
        assert d.last_ms() > 0.0 and d.vertices_ptr and d.normals_ptr
        d.close()


@pytest.mark.gpu
def test_pose_over_more_tiles_than_the_staged_grid_has_workgroups(cr, palette):
    """2048 workgroups stride over the tiles in the LDS form: 2049 tiles of vertices and one of normals, no targets"""
    nv = 2048 * 256 + 1
    rng = np.random.default_rng(17)
    rest = rng.uniform(-2, 2, (nv, 3)).astype(f32)
    vb, vw = rng.integers(0, 16, (nv, 4)).astype(np.uint16), _weights(rng, nv)
    n = rng.normal(size=(100, 3)).astype(f32)
    nb, nw = rng.integers(0, 16, (100, 4)).astype(np.uint16), _weights(rng, 100)
    bones = rng.normal(size=(16, 3, 4)).astype(f32)
    d = cr.Deformer(rest, vb, vw, n, nb, nw, n_bones=16)
    d.pose(bones)
    _equal(d.read(), deform_ref(bones, rest, vb, vw, n, nb, nw))
    d.close()


@pytest.mark.gpu
def test_deformer_without_normals_and_refused_poses(cr):
    from caitlynrenderer_amd import _lib
    case, bones, mw = make_case(21, 257, 7)
    plain = {k: case[k] for k in ("rest_vertices", "vertex_bones", "vertex_weights", "morph_targets")}
    d = cr.Deformer(n_bones=7, **plain)
    with pytest.raises(cr.CrtError):
        d.read()                                              # no pose yet
    d.pose(bones, mw)
    want = deform_ref(bones, morph_weights=mw, **plain)
    _equal(d.read(), want)
    assert d.normals_ptr is None
    for b, w in ((np.where(np.arange(84).reshape(7, 3, 4) == 40, np.nan, bones).astype(f32), mw), (bones, np.array([0, 0, np.inf, 0, 0], f32))):
        with pytest.raises(cr.CrtError) as e:
            d.pose(b, w)
        assert e.value.code == _lib.CRT_ERR_INVALID
        _equal(d.read(), want)                                # the outputs as they were
    d.close()


def _accel(scene):
    return [scene.debug_read_accel(k) for k in range(4)]


def _frames(scene, rvs):
    scene.render_frame(*rvs[0])
    scene.render_frames(rvs[1:])
    return scene.read_sum().copy()


def _scene_rig(cr, mesh, seed, n_bones=5):
    """A rig for a fixture mesh: smooth four-bone weights along y, morph targets, and two poses of small rotations and translations"""
    rng = np.random.default_rng(seed)
    V = np.ascontiguousarray(mesh.vertices, f32)
    nv = V.shape[0]
    y = (V[:, 1] - V[:, 1].min()) / max(float(np.ptp(V[:, 1])), 1e-6) * (n_bones - 1)
    b0 = np.clip(np.floor(y).astype(np.int64) - 1, 0, n_bones - 4)
    vb = (b0[:, None] + np.arange(4)).astype(np.uint16)
    w = np.exp(-(y[:, None] - vb) ** 2).astype(f32)
    vw = (w / w.sum(1, keepdims=True)).astype(f32)
    vw[::5, 3] = 0.0
    nb, nw = cr.normal_influences(mesh.triangles, vb, vw, mesh.normals.shape[0])
    targets = []
    for t in range(2):
        idx = np.nonzero(rng.random(nv) < 0.4)[0].astype(np.uint32)
        targets.append((idx, rng.normal(scale=0.01, size=(idx.shape[0], 3)).astype(f32)))
    case = dict(rest_vertices=V, vertex_bones=vb, vertex_weights=vw, rest_normals=mesh.normals, normal_bones=nb, normal_weights=nw, morph_targets=targets)
    poses = []
    for k in range(2):
        B = np.tile(IDENTITY, (n_bones, 1, 1))
        for i in range(n_bones):
            a = 0.05 * (k + 1) * (i - 2)
            B[i, :, :3] = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]], f32)
            B[i, :, 3] = rng.normal(scale=0.01, size=3)
        poses.append((B.astype(f32), rng.uniform(0, 1, 2).astype(f32)))
    return case, poses


def _same_scene(cr, mesh, a, b, seed, rvs):
    for k in range(4):
        assert np.array_equal(_bits(a.debug_read_accel(k)), _bits(b.debug_read_accel(k))), k
    rays = seeded_rays(mesh, 2048, seed, cr.RAY_DT)
    assert np.array_equal(_bits(a.trace(rays)), _bits(b.trace(rays)))
    fa, fb = _frames(a, rvs), _frames(b, rvs)
    assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32)) and fa.max() > 0.0


RVS = [(RX1, RY1), (0.3, 0.7)]


@pytest.mark.gpu
@pytest.mark.parametrize("fixture", ["cornell", "tess8"])
@pytest.mark.parametrize("mode", ["refit", "refit_async", "keep_normals", "rebuild"])
def test_scene_deform_equals_update_vertices_with_the_reference_arrays(cr, cornell, tess8, fixture, mode):
    mesh = cornell[0] if fixture == "cornell" else tess8[0]
    if mode == "rebuild":
        data = cr.SceneData.for_device_build(mesh, cornell[1], builder="sah")
    else:
        data = cr.SceneData.build(mesh, cornell[1])
    case, poses = _scene_rig(cr, mesh, 31)
    d = cr.Deformer(n_bones=5, **case)
    a, b = cr.Scene(data, 64, 64, 3), cr.Scene(data, 64, 64, 3)
    for k, (bones, mw) in enumerate(poses):
        V, N = deform_ref(bones, morph_weights=mw, **case)
        assert not np.array_equal(N, mesh.normals)
        if mode == "rebuild":
            a.deform(d, bones, mw, rebuild=True)
            b.rebuild_vertices(V, N)
        elif mode == "keep_normals":
            a.deform(d, bones, mw, keep_normals=True)
            b.update_vertices(V)
        else:
            a.deform(d, bones, mw, sync=(mode == "refit"))
            b.update_vertices(V, N)
        _same_scene(cr, mesh, a, b, 40 + k, RVS)
        _equal(d.read(), (V, N))
    assert a.last_update_ms()[0] > 0.0 and d.last_ms() > 0.0
    # the deformer's own stream orders itself behind the scene's: a pose right after an unsynchronised deform
    a.deform(d, *poses[0], sync=False)
    d.pose(*poses[1])
    _equal(d.read(), deform_ref(poses[1][0], morph_weights=poses[1][1], **case))
    a.close(); b.close(); d.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bad", ["vertex count", "normal count", "nan bone", "far bone", "flags", "rebuild of a host-built scene"])
def test_a_refused_deform_leaves_the_scene_as_it_was(cr, tess8, cornell, bad):
    from caitlynrenderer_amd import _lib
    mesh, data = tess8
    case, poses = _scene_rig(cr, mesh, 32)
    bones, mw = poses[0]
    bones = bones.copy()
    kw = {}
    if bad == "vertex count":
        case = dict(case, rest_vertices=case["rest_vertices"][:-1], vertex_bones=case["vertex_bones"][:-1], vertex_weights=case["vertex_weights"][:-1],
                    morph_targets=None)
        mw = None
    elif bad == "normal count":
        case = dict(case, rest_normals=case["rest_normals"][:-1], normal_bones=case["normal_bones"][:-1], normal_weights=case["normal_weights"][:-1])
    elif bad == "nan bone":
        bones[3, 1, 1] = np.nan
    elif bad == "far bone":
        bones[2, 0, 3] = 3e18
    elif bad == "rebuild of a host-built scene":
        kw["rebuild"] = True
    d = cr.Deformer(n_bones=5, **case)
    sc, ref = cr.Scene(data, 64, 64, 3), cr.Scene(data, 64, 64, 3)
    sc.render_frame(RX1, RY1); ref.render_frame(RX1, RY1)
    a0 = _accel(sc)
    if bad == "flags":
        b = np.ascontiguousarray(bones).reshape(-1)
        assert _lib.lib().crt_deform_scene(sc._h, d._h, b.ctypes.data, mw.ctypes.data, 4, 1) == _lib.CRT_ERR_INVALID
    else:
        with pytest.raises(cr.CrtError) as e:
            sc.deform(d, bones, mw, **kw)
        assert e.value.code == _lib.CRT_ERR_INVALID and "crt_deform_scene: " in str(e.value)
    for k in range(4):
        assert np.array_equal(_bits(sc.debug_read_accel(k)), _bits(a0[k])), k
    rvs = [(0.3, 0.7), (0.1, 0.2)]
    assert np.array_equal(_frames(sc, rvs).view(np.uint32), _frames(ref, rvs).view(np.uint32))
    if bad == "normal count":                                  # the same deformer is taken with the scene's normals kept
        sc.deform(d, bones, mw, keep_normals=True)
        ref.update_vertices(deform_ref(bones, morph_weights=mw, **case)[0])
        assert np.array_equal(_frames(sc, rvs).view(np.uint32), _frames(ref, rvs).view(np.uint32))
    sc.close(); ref.close(); d.close()


@pytest.mark.gpu
def test_deform_refuses_an_instanced_scene(cr, cornell):
    from caitlynrenderer_amd import _lib
    mesh = cornell[0]
    case, poses = _scene_rig(cr, mesh, 33)
    d = cr.Deformer(n_bones=5, **case)
    inst = cr.InstancedScene([mesh], cr.instances_array(IDENTITY[None], [0]))
    sc = inst.frame_scene([mesh], mesh.materials, mesh.lights, 64, 64, 3)
    sc.update(cornell[1])
    sc.render_frame(RX1, RY1)
    before = sc.read_sum().copy()
    with pytest.raises(cr.CrtError) as e:
        sc.deform(d, *poses[0])
    assert e.value.code == _lib.CRT_ERR_INVALID and "instanced" in str(e.value)
    assert np.array_equal(sc.read_sum().view(np.uint32), before.view(np.uint32))
    sc.close(); inst.close(); d.close()


@pytest.mark.gpu
def test_posed_meshes_into_an_instanced_handle(cr, cornell, tess8):
    """pose, then crt_instances_update_meshes_device with the deformer's pointer, against crt_instances_update_meshes with the reference's array"""
    meshes = [cornell[0], tess8[0]]
    M = np.stack([IDENTITY, IDENTITY, IDENTITY])
    M[1, :, 3], M[2, :, 3] = (3, 0, 0), (0, 0, -3)
    inst = cr.instances_array(M, [0, 1, 0])
    a = cr.InstancedScene(meshes, inst, updatable=True)
    b = cr.InstancedScene(meshes, inst, updatable=True)
    rigs = [_scene_rig(cr, m, 50 + k) for k, m in enumerate(meshes)]
    ds = [cr.Deformer(n_bones=5, **{k: v for k, v in case.items() if "normal" not in k}) for case, _ in rigs]
    want = {}
    for k, ((case, poses), d) in enumerate(zip(rigs, ds)):
        d.pose(*poses[1])                                      # synchronised: the handle reads on a stream of its own
        want[k] = deform_ref(poses[1][0], morph_weights=poses[1][1], **case)[0]
    a.update_meshes_device({k: (d.vertices_ptr, d.n_vertices) for k, d in enumerate(ds)})
    b.update_meshes(want)
    rng = np.random.default_rng(9)
    rays = np.zeros(4096, cr.RAY_DT)
    rays["o"] = rng.uniform(-1, 4, (4096, 3)).astype(f32)
    dirs = rng.normal(size=(4096, 3))
    rays["d"] = (dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(f32)
    rays["tmax"] = f32(1e9)
    (ha, ia), (hb, ib) = a.trace(rays), b.trace(rays)
    assert np.array_equal(_bits(ha), _bits(hb)) and np.array_equal(ia, ib) and (ia >= 0).sum() > 1000
    a.close(); b.close()
    for d in ds:
        d.close()
