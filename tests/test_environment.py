"""Environment lighting (crt_set_environment) held to tests/env_ref.py: the definition of include/crt.h restated in float32
numpy, and integrator_ref's loop with the one miss line added.  The C oracle has no environment.

CPU cases: env_ref.render with env = None is integrator_ref.render by bits on every scene used below (flat, instanced, through a lens);
E(d) at the six axes of a six-colour map, through a rotation that permutes the axes too; E is continuous across the octahedral edges and
corners (and a clamp-only tap is not); octahedral_from_equirect against octahedral_from_function; the census condition — every case
compared on the GPU reaches the new code.  GPU cases: frames as uint32 words with their ray counts and resolved bytes, every other way to
the same frame, instanced scenes, a furnace that does not lean on the restated loop, the way back to the parent's frames, the feature
buffers, the denoiser and the temporal filter, and the refusals.

All comparisons of frames are exact.  The bounds of the other tests are derived where they stand."""
import ctypes as C
import types

import numpy as np
import pytest

import env_ref as er
import integrator_ref as ir
import lens_ref as lr

f32 = np.float32
W, H = 44, 28               # conftest's small frame: no multiple of the 8-, 16- or 64-pixel tiles; W != H
FRAMES = 4
E_CONST = (0.5, 1.0, 2.0)
FACE_ALBEDO = np.array([(0.8, 0.3, 0.2), (0.2, 0.7, 0.3), (0.3, 0.4, 0.9), (0.7, 0.7, 0.2), (0.6, 0.2, 0.7), (0.25, 0.65, 0.7)], f32)
LENS = {"modest": (f32(0.03), f32(3.0)), "hostile": (f32(0.5), f32(0.5))}


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the scenes, built by hand

def lambert(albedo, kind=0.0, emission=None, light=-1.0):
    m = np.full(16, -1.0, f32)
    m[0:3], m[3] = albedo, kind
    m[4:7], m[7] = (0, 0, 0) if emission is None else emission, light
    m[8:12] = 0.0
    return m


def cube_rows(centre, first_vertex, first_material):
    """the unit cube about `centre`: 12 triangles with FLAT integer normals (vn.w == 0), face k of material first_material + k"""
    lo, hi = np.asarray(centre, np.float64) - 0.5, np.asarray(centre, np.float64) + 0.5
    v, t = [], []
    for axis in range(3):
        for side in (0, 1):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            c = [np.zeros(3) for _ in range(4)]
            for k, (sa, sb) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
                c[k][axis] = (hi if side else lo)[axis]
                c[k][a] = (hi if sa else lo)[a]
                c[k][b] = (hi if sb else lo)[b]
            i = first_vertex + len(v)
            v += c
            n = [0, 0, 0]
            n[axis] = 1 if side else -1
            mtl = first_material + 2 * axis + side
            t += [[i, i + 1, i + 2, mtl] + n + [0, -1, -1, -1, 0], [i, i + 2, i + 3, mtl] + n + [0, -1, -1, -1, 0]]
    return v, t


def quad_rows(p, a, b, first_vertex, mtl, normal):
    p, a, b = (np.asarray(x, np.float64) for x in (p, a, b))
    i = first_vertex
    return [p, p + a, p + a + b, p + b], [[i, i + 1, i + 2, mtl] + list(normal) + [0, -1, -1, -1, 0], [i, i + 2, i + 3, mtl] + list(normal) + [0, -1, -1, -1, 0]]


def mesh_of(cr, v, t, mats, lights=None):
    return cr.Mesh(np.array(v, f32), np.zeros((0, 3), f32), np.zeros((0, 2), f32), np.array(t, np.int32), np.array(mats, f32),
                   np.zeros((0, 18), f32) if lights is None else np.array(lights, f32))


def cube_scene(cr):
    """(a) the unit cube about the origin, per-face Lambert albedos, on nothing"""
    v, t = cube_rows((0, 0, 0), 0, 0)
    return mesh_of(cr, v, t, [lambert(a) for a in FACE_ALBEDO]), cr.Camera((1.6, 1.2, -2.2), (0.0, 0.0, 0.0), 45.0)


def cube_quad_scene(cr):
    """(b) that cube over a ground quad (a hair below its bottom face: no two surfaces at one t) with one emissive triangle above, facing
    down: NEE, MIS and the environment act in one path"""
    v, t = cube_rows((0, 0, 0), 0, 0)
    mats = [lambert(a) for a in FACE_ALBEDO] + [lambert((0.6, 0.6, 0.55)), lambert((0, 0, 0), emission=(7.0, 6.0, 5.0), light=0.0)]
    qv, qt = quad_rows((-3, -0.51, -3), (0, 0, 6), (6, 0, 0), len(v), 6, (0, 1, 0))
    v, t = v + qv, t + qt
    lamp = [np.array(p, np.float64) for p in ((-0.6, 2.0, -0.4), (0.6, 2.0, -0.4), (0.0, 2.0, 0.7))]
    i = len(v)
    v += lamp
    t.append([i, i + 1, i + 2, 7, 0, -1, 0, 0, -1, -1, -1, 0])
    u_, v_ = lamp[1] - lamp[0], lamp[2] - lamp[0]
    area = float(np.linalg.norm(np.cross(u_, v_)))
    light = np.concatenate([lamp[0], u_, v_, (0, -1, 0), (7.0, 6.0, 5.0), (area, 1.0, 0.0)])
    return mesh_of(cr, v, t, mats, [light]), cr.Camera((2.2, 1.6, -3.0), (0.0, 0.0, 0.0), 50.0)


def mirror_scene(cr):
    """(c) a Mirror quad facing the sky with the cube hovering over a corner of it: special_materials, specular misses"""
    v, t = cube_rows((0.5, 1.0, 0.4), 0, 0)
    mats = [lambert(a) for a in FACE_ALBEDO] + [lambert((0.9, 0.9, 0.9), kind=1.0)]
    qv, qt = quad_rows((-1.5, 0, -1.5), (0, 0, 3), (3, 0, 0), len(v), 6, (0, 1, 0))
    return mesh_of(cr, v + qv, t + qt, mats), cr.Camera((0.0, 2.5, -3.5), (0.0, 0.3, 0.0), 50.0)


def outside_camera(cr, mesh):
    lo, hi = mesh.vertices.min(0).astype(np.float64), mesh.vertices.max(0).astype(np.float64)
    c, r = (lo + hi) / 2, float(np.linalg.norm(hi - lo))
    return cr.Camera(tuple(c + r * np.array([0.9, 0.5, -1.3])), tuple(c), 45.0)


# ---------------------------------------------------------------------------------------------- the environments

def six_colour(d):
    """the colour of the dominant axis of d: +x red, -x cyan, +y green, -y magenta, +z blue, -z yellow"""
    table = np.array([[(0, 1, 1), (1, 0, 0)], [(1, 0, 1), (0, 1, 0)], [(1, 1, 0), (0, 0, 1)]], np.float64)
    k = np.argmax(np.abs(d), axis=1)
    return table[k, (d[np.arange(d.shape[0]), k] > 0).astype(np.int64)]


def gradient(d):
    return 0.25 * (d + 1.0)


def rotation_matrix(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return (np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)).astype(f32)


@pytest.fixture(scope="module")
def envs(cr):
    from caitlynrenderer_amd.environment import constant_environment, octahedral_from_function
    map16 = octahedral_from_function(lambda d: six_colour(d) + gradient(d), 16)
    R = rotation_matrix((1, 2, 3), 0.7)
    return {"map16": er.Env(map16, R, (0.8, 1.1, 0.6)), "map16_hide": er.Env(map16, R, (0.8, 1.1, 0.6), hide_from_camera=True),
            "const1": er.Env(constant_environment(E_CONST)), "zero": er.Env(map16, R, (0.0, 0.0, 0.0))}


def set_env(scene, env):
    scene.set_environment(env.texels, env.rotation, tuple(float(x) for x in env.scale), env.hide_from_camera)


# ---------------------------------------------------------------------------------------------- shared, computed once

@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def cases(cr, tess8, textured):
    """name -> (mesh, SceneData, camera)"""
    out = {}
    for name, make in (("cube", cube_scene), ("cube_quad", cube_quad_scene), ("mirror", mirror_scene)):
        mesh, cam = make(cr)
        out[name] = (mesh, cr.SceneData.build(mesh, cam), cam)
    out["tess8"] = (tess8[0], tess8[1], outside_camera(cr, tess8[0]))
    out["textured"] = (textured[0], textured[1], outside_camera(cr, textured[0]))
    return out


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make(key)
        return self[key]


def _frozen(sums):
    for s in sums:
        s.setflags(write=False)
    return sums


def primary_of(view):
    """view: "pinhole", "nojitter", or a key of LENS -> the `primary` env_ref.render takes"""
    if view == "pinhole":
        return None
    if view == "nojitter":
        return lambda sc, rx, ry: ir.primary_rays(sc, rx, ry, jitter=False)

    def through_lens(sc, rx, ry):
        out = lr.lens_rays(sc, rx, ry, *LENS[view])
        return out["o"].copy(), out["d"].copy(), out["rng"], out["census"]
    return through_lens


@pytest.fixture(scope="module")
def reference(cases, envs, rvs):
    """(scene, environment, view, depth) -> (sums[k - 1] for k <= depth, per-frame census [frame][k - 1], census over the frames)"""
    def make(key):
        name, env, view, depth = key
        mesh, _, cam = cases[name]
        sums, _, total, per_frame = er.render(ir.RefScene(mesh, cam, W, H), rvs, depth, envs[env] if env else None, primary_of(view))
        return _frozen(sums), per_frame, total
    return _Lazy(make)


def lens_camera(cr, cam, aperture, focal_dist):
    from caitlynrenderer_amd._lib import crt_camera
    c = crt_camera()
    C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(crt_camera))
    c.aperture, c.focal_dist = float(aperture), float(focal_dist)
    return types.SimpleNamespace(c=c)


# every (scene, environment, depth) whose frames are compared on the GPU against env_ref
GPU_CASES = [(n, "map16", d) for n in ("cube", "cube_quad", "mirror", "textured", "tess8") for d in (1, 2, 3)] + \
            [("cube_quad", "map16", 16), ("cube_quad", "map16_hide", 3), ("mirror", "map16_hide", 2), ("cube_quad", "const1", 3), ("cube", "const1", 2)]


def ref_depth(depth):
    return 16 if depth > 3 else 3       # one run at 3 gives 1 and 2 as well


# ---------------------------------------------------------------------------------------------- CPU: the copy of the loop has not drifted

def same_four(a, b):
    for x, y in zip(a[0], b[0]):
        assert np.array_equal(bits(x), bits(y))
    for fa, fb in zip(a[1], b[1]):
        for x, y in zip(fa, fb):
            assert np.array_equal(bits(x), bits(y))
    assert a[2] == b[2] and a[3] == b[3]


@pytest.mark.parametrize("name", ("cube", "cube_quad", "mirror", "textured", "tess8"))
def test_no_environment_is_integrator_ref_by_bits(cases, rvs, name):
    mesh, _, cam = cases[name]
    scene = ir.RefScene(mesh, cam, W, H)
    depth = 3 if name in ("tess8", "textured") else 4
    same_four(er.render(scene, rvs[:2], depth, None), ir.render(scene, rvs[:2], depth))


def test_no_environment_is_lens_ref_by_bits(cases, rvs):
    mesh, _, cam = cases["cube_quad"]
    scene = ir.RefScene(mesh, cam, W, H)
    for view in LENS:
        same_four(er.render(scene, rvs[:2], 3, None, primary_of(view)), lr.render(scene, rvs[:2], 3, *LENS[view]))
    # option "jitter" 0: integrator_ref.render over its own primary rays without the jitter
    from unittest import mock
    plain = ir.primary_rays
    with mock.patch.object(ir, "primary_rays", lambda sc, rx, ry, jitter=True: plain(sc, rx, ry, jitter=False)):
        want = ir.render(scene, rvs[:2], 3)
    same_four(er.render(scene, rvs[:2], 3, None, primary_of("nojitter")), want)


def yard_ref(cr, masks):
    import instanced_ref as xr
    from test_lens import INST_MASKS, lens_yard
    s = lens_yard(cr)
    return s, xr.InstancedRef(s.meshes, s.M, s.mesh_of, s.masks, s.offsets, s.mats, s.static, s.mesh_lights, s.textures, s.cam, W, H,
                              options=INST_MASKS if masks else None)


def test_no_environment_is_instanced_ref_by_bits(cr, rvs):
    for masks in (False, True):
        _, ref = yard_ref(cr, masks)
        same_four(er.render(ref, rvs[:2], 3, None), ir.render(ref, rvs[:2], 3))


# ---------------------------------------------------------------------------------------------- CPU: E(d)

AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)], f32)


@pytest.mark.parametrize("size", (16, 5, 4))
def test_six_axes_of_a_six_colour_map(cr, size):
    """The four taps around the image of an axis all lie in that axis' region of a six-colour map of size >= 4 (a 2 x 2 map has four texels for six colours), so E is its colour up to
    the blend's three roundings (1e-6 of values <= 1).  The permutation sends world x -> map y -> ..., and the colours follow."""
    from caitlynrenderer_amd.environment import octahedral_from_function
    texels = octahedral_from_function(six_colour, size)
    want = six_colour(AXES.astype(np.float64))
    got = er.radiance(er.Env(texels), AXES)
    assert np.abs(got - want).max() <= 1e-6, got
    P = np.array([[0, 1, 0], [0, 0, 1], [1, 0, 0]], f32)
    got = er.radiance(er.Env(texels, P, (2.0, 0.5, 1.0)), AXES)
    assert np.abs(got - six_colour((AXES @ P.T).astype(np.float64)) * np.array([2.0, 0.5, 1.0])).max() <= 2e-6, got
    # not (s > 0) and s not finite: no radiance
    bad = np.array([(0, 0, 0), (np.inf, 0, 0), (np.nan, 1, 0)], f32)
    assert not er.radiance(er.Env(texels), bad).any()


def neighbour_bound(env):
    """the largest difference between two texels that are neighbours on the octahedron: taps (i, j), (i + 1, j) and (i, j), (i, j + 1) for
    i, j from -1 to size - 1, the edge identification included"""
    idx = np.arange(-1, env.size)
    i, j = (x.reshape(-1) for x in np.meshgrid(idx, idx, indexing="ij"))
    a = er._tap(env, i, j)
    return float(max(np.abs(er._tap(env, i + 1, j) - a).max(), np.abs(er._tap(env, i, j + 1) - a).max()))


def straddling_pairs():
    """pairs of unit directions 1e-4 apart: across the four edges of the square — the arcs y = 0 and x = 0 of the lower hemisphere, three
    points each — and around -z, where the four corners meet, one pair for every two of the four quadrants"""
    h = 5e-5
    out = []
    for z in (-0.25, -0.6, -0.9):
        r = np.sqrt(1 - z * z)
        for sgn in (1, -1):
            out += [((sgn * r, h, z), (sgn * r, -h, z)), ((h, sgn * r, z), (-h, sgn * r, z))]
    q = [(h, h), (-h, h), (-h, -h), (h, -h)]
    out += [((q[a][0] / np.sqrt(2), q[a][1] / np.sqrt(2), -1.0), (q[b][0] / np.sqrt(2), q[b][1] / np.sqrt(2), -1.0)) for a in range(4) for b in range(a + 1, 4)]
    a = np.array([p[0] for p in out], np.float64)
    b = np.array([p[1] for p in out], np.float64)
    return a / np.linalg.norm(a, axis=1, keepdims=True), b / np.linalg.norm(b, axis=1, keepdims=True)


def test_radiance_is_continuous_across_the_octahedral_edges(cr):
    """With p = e / |e|_1, the Jacobian of d -> p has norm <= 1 / s + |e|_2 |sgn|_2 / s^2 <= 1 + sqrt(3) (s >= 1 on unit vectors), the fold
    of the lower hemisphere moves neither coordinate faster than p moves, and (fx, fy) = p size / 2 + const.  On the square with its edges
    identified the bilinear interpolant is continuous and piecewise bilinear with slopes <= G per texel in either coordinate, G the largest
    difference between neighbouring texels.  So |E(a) - E(b)| <= 2 G (1 + sqrt 3) (size / 2) |a - b|, plus the float32 evaluation's own
    error: a dozen roundings of values <= max E on either side, 32 ulp in all.  Clamp-only taps break this at every edge pair."""
    from caitlynrenderer_amd.environment import octahedral_from_function
    smooth = lambda d: 1.0 + 0.5 * np.stack([d[:, 0] * 0.8 + d[:, 1] * 0.6, d[:, 1] * 0.6 - d[:, 2] * 0.8, np.sin(2.0 * d[:, 0]) * d[:, 2]], -1)
    for size in (16, 7):
        env = er.Env(octahedral_from_function(smooth, size))
        a, b = straddling_pairs()
        dist = np.linalg.norm(a.astype(f32).astype(np.float64) - b.astype(f32).astype(np.float64), axis=1)
        G = neighbour_bound(env)
        bound = 2.0 * G * (1.0 + np.sqrt(3.0)) * (size / 2.0) * dist + 32 * 2.0 ** -24 * float(env.texels.max())
        delta = np.abs(er.radiance(env, a).astype(np.float64) - er.radiance(env, b).astype(np.float64)).max(1)
        print(size, "G", G, "worst |dE| / bound", float((delta / bound).max()))
        assert (delta <= bound).all(), (size, delta / bound)
        broken = np.abs(er.radiance(env, a, clamp_only=True).astype(np.float64) - er.radiance(env, b, clamp_only=True).astype(np.float64)).max(1)
        assert (broken[:12] > bound[:12]).sum() >= 8, broken[:12] / bound[:12]       # the edge pairs: a clamp-only tap jumps


def test_equirect_resampling_agrees_with_the_function(cr):
    """g is 1 + 0.5 a.d per channel: along either angle its second derivative is at most 0.5, so a bilinear lookup in a W x H lat-long
    grid is off by at most (1 / 8) (0.5 (2 pi / W)^2 + 0.5 (pi / H)^2) = 3.0e-4 at 128 x 64, away from the clamped half row at either pole
    (0.0245 rad; the nearest octahedral texel centre of a size-16 map is 0.066 rad from a pole).  float32 texels add 1e-7."""
    from caitlynrenderer_amd.environment import equirect_lookup, octahedral_from_equirect, octahedral_from_function
    A = np.array([(0.8, 0.6, 0.0), (0.0, 0.6, -0.8), (-0.6, 0.0, 0.8)])
    g = lambda d: 1.0 + 0.5 * d @ A.T
    Wl, Hl = 128, 64
    for up in ("y", "z"):
        k = {"y": 1, "z": 2}[up]
        v, u = np.meshgrid((np.arange(Hl) + 0.5) / Hl * np.pi, (np.arange(Wl) + 0.5) / Wl * 2 * np.pi, indexing="ij")
        d = np.zeros((Hl, Wl, 3))
        d[..., k], d[..., (k + 1) % 3], d[..., (k + 2) % 3] = np.cos(v), np.sin(v) * np.cos(u), np.sin(v) * np.sin(u)
        img = g(d.reshape(-1, 3)).reshape(Hl, Wl, 3)
        assert np.abs(equirect_lookup(img, d.reshape(-1, 3), up) - img.reshape(-1, 3)).max() < 1e-9       # the texel centres return their texels
        got, want = octahedral_from_equirect(img, 16, up=up), octahedral_from_function(g, 16)
        bound = (0.5 * (2 * np.pi / Wl) ** 2 + 0.5 * (np.pi / Hl) ** 2) / 8 + 1e-6
        print(up, "worst", float(np.abs(got - want).max()), "bound", bound)
        assert got.shape == (16, 16, 3) and got.dtype == f32 and np.abs(got - want).max() <= bound


def test_helpers_shapes(cr):
    from caitlynrenderer_amd.environment import constant_environment, octahedral_directions
    d = octahedral_directions(4)
    assert d.shape == (4, 4, 3) and np.allclose(np.linalg.norm(d, axis=-1), 1.0)
    assert (d[1:3, 1:3, 2] > 0).all() and (d[0, 0, 2] < 0) and (d[3, 3, 2] < 0)           # +z in the middle, -z at the corners
    assert d[0, 1, 1] < 0 and d[3, 1, 1] > 0                                              # row 0 is the lowest py
    c = constant_environment(E_CONST)
    assert c.shape == (1, 1, 3) and c.dtype == f32
    assert np.abs(er.radiance(er.Env(c), AXES) - np.array(E_CONST)).max() <= 1e-6


# ---------------------------------------------------------------------------------------------- CPU: the census condition

@pytest.mark.parametrize("name,env,depth", GPU_CASES)
def test_every_gpu_case_reaches_the_new_code(reference, name, env, depth):
    _, _, total = reference[(name, env, "pinhole", ref_depth(depth))]
    c = total[depth - 1]
    print(name, env, depth, "miss_first", c["miss_first"], "miss_later", c["miss_later"])
    assert c["miss_first"] > 0
    if depth >= 2:
        assert c["miss_later"] > 0 and 10 * (c["miss_first"] + c["miss_later"]) >= W * H * FRAMES


def test_instanced_reference_reaches_the_new_code(inst_reference):
    for masks in (False, True):
        for depth in (1, 3):
            c = inst_reference[masks][2][depth - 1]
            assert c["miss_first"] > 0
            if depth >= 2:
                assert c["miss_later"] > 0 and 10 * (c["miss_first"] + c["miss_later"]) >= W * H * FRAMES


def test_an_environment_changes_the_frames(reference):
    lit, dark = reference[("cube_quad", "map16", "pinhole", 3)][0][2], reference[("cube_quad", None, "pinhole", 3)][0][2]
    assert int((bits(lit) != bits(dark)).sum()) >= lit.size // 4
    hidden = reference[("cube_quad", "map16_hide", "pinhole", 3)][0]
    assert np.array_equal(bits(hidden[0]), bits(reference[("cube_quad", None, "pinhole", 3)][0][0]))     # depth 1, hidden: nothing to see
    assert int((bits(hidden[2]) != bits(lit)).sum()) > 0 and int((bits(hidden[2]) != bits(dark)).sum()) > 0


# ---------------------------------------------------------------------------------------------- GPU: frames

def render_and_check(cr, data, cam, env, entry, rvs, depth, options=(), one_call=False, devices=None, expect_samples=None, lens=None, counts_only=False, devices_late=None):
    sums, per_frame, total = entry
    scene = cr.Scene(data, W, H, depth)
    try:
        if devices is not None:
            scene.set_devices(devices)
        for k, v in options:
            scene.set_option(k, v)
        if lens is not None:
            scene.update(lens_camera(cr, cam, *lens))
        else:
            scene.update(cam)
        set_env(scene, env)
        if devices_late is not None:                     # the devices' replicas are made from a scene that has its environment already
            scene.set_devices(devices_late)
        form = 32 | (16 if lens is not None else 0)
        if one_call:
            scene.render_frames(rvs)
            st = scene.frame_stats()
            info = scene.launch_info()
            assert info[0] == 0 and info[1] == form and info[2] == expect_samples, info
            if info[2] == len(rvs):
                assert (st["closest_rays"], st["any_rays"]) == (total[depth - 1]["closest_rays"], total[depth - 1]["shadow_rays"])
        else:
            for f, (rx, ry) in enumerate(rvs):
                scene.render_frame(rx, ry)
                st = scene.frame_stats()
                assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
            info = scene.launch_info()
            assert info[:3] == [0, form, 1], info
        assert st["stack_overflows"] == 0
        if counts_only:
            return
        got = scene.read_sum()
        differing = int((bits(got) != bits(sums[depth - 1])).sum())
        assert differing == 0, differing
        scene.frame_count = len(rvs)
        rgba = scene.resolve()
        assert np.array_equal(rgba, ir.resolve_ref(got, f32(1.0 / len(rvs))))
        assert np.array_equal(rgba, ir.resolve_ref(sums[depth - 1], f32(1.0 / len(rvs))))
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name,env,depth", GPU_CASES)
def test_gpu_frames_equal_the_reference(cr, cases, envs, rvs, reference, name, env, depth):
    """the sums after four render_frame calls as uint32 words, each frame's closest and shadow ray counts against the census, and the
    resolved bytes against resolve_ref"""
    _, data, cam = cases[name]
    render_and_check(cr, data, cam, envs[env], reference[(name, env, "pinhole", ref_depth(depth))], rvs, depth)


VARIANTS = ("lens_modest", "lens_hostile", "render_frames", "render_frames_lens", "two_devices", "two_devices_late", "streams_2", "jitter_0", "count_visits_1", "device_built_sah",
            "inplace_shadow_0", "inplace_shadow_1", "inplace_shadow_2", "bounce_refill_0", "bounce_refill_1")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_variants_equal_the_reference(cr, cases, envs, rvs, reference, variant):
    """the cube on its quad under the 16 x 16 map, paths of 3 segments, once through each other way to the same frame"""
    name, depth, kw, view = "cube_quad", 3, {}, "pinhole"
    data = cases[name][1]
    if variant.startswith("lens_"):
        view = variant[5:]
        kw = {"lens": LENS[view]}
    elif variant == "render_frames":
        kw = {"one_call": True, "expect_samples": 1}                 # a pinhole: one sample per chain
    elif variant == "render_frames_lens":
        view, kw = "modest", {"one_call": True, "expect_samples": FRAMES, "lens": LENS["modest"]}
    elif variant == "two_devices":
        kw = {"devices": [0, 0]}
    elif variant == "two_devices_late":
        kw = {"devices_late": [0, 0]}
    elif variant == "streams_2":
        kw = {"options": (("streams", 2),)}
    elif variant == "jitter_0":
        view, kw = "nojitter", {"options": (("jitter", 0),)}
    elif variant == "count_visits_1":
        kw = {"options": (("count_visits", 1),), "counts_only": True}
    elif variant == "device_built_sah":
        data = cr.SceneData.for_device_build(cases[name][0], cases[name][2], "sah")
    else:
        k, v = variant.rsplit("_", 1)
        kw = {"options": ((k, int(v)),)}
    render_and_check(cr, data, cases[name][2], envs["map16"], reference[(name, "map16", view, 3)], rvs, depth, **kw)


@pytest.mark.gpu
def test_gpu_tile_shards_add_up_to_the_frame(cr, cases, envs, rvs, reference):
    _, data, cam = cases["cube_quad"]
    want = reference[("cube_quad", "map16", "pinhole", 3)][0][2]
    got = np.zeros((H, W, 3), f32)
    covered = np.zeros((H, W), np.int64)
    for rank in (0, 1):
        scene = cr.Scene(data, W, H, 3)
        try:
            scene.set_shard(rank, 2, 8)
            scene.update(cam)
            set_env(scene, envs["map16"])
            for rx, ry in rvs:
                scene.render_frame(rx, ry)
            part = scene.read_sum()
            got += part
            covered += (part != 0).any(-1)
        finally:
            scene.close()
    assert covered.max() == 1 and np.array_equal(bits(got), bits(want + f32(0.0)))


# ---------------------------------------------------------------------------------------------- GPU: instanced scenes

@pytest.fixture(scope="module")
def inst_reference(cr, rvs, envs):
    def make(masks):
        s, ref = yard_ref(cr, masks)
        sums, _, total, per_frame = er.render(ref, rvs, 3, envs["map16"])
        return _frozen(sums), per_frame, total, s
    return _Lazy(make)


@pytest.mark.gpu
@pytest.mark.parametrize("masks", (False, True))
@pytest.mark.parametrize("depth", (1, 3))
def test_gpu_instanced_frames_equal_the_reference(cr, inst_reference, envs, rvs, depth, masks):
    from test_instances_frames import shading_of
    from test_lens import INST_MASKS
    sums, per_frame, _, s = inst_reference[masks]
    inst = cr.InstancedScene(s.meshes, cr.instances_array(s.M, s.mesh_of, masks=s.masks, material_offsets=s.offsets), builder="sah")
    sc = inst.frame_scene(shading_of(s.meshes), s.mats, s.static, W, H, depth, textures=None, mesh_lights=s.mesh_lights)
    try:
        for k, v in (INST_MASKS if masks else {}).items():
            sc.set_option(k, v)
        sc.update(s.cam)
        set_env(sc, envs["map16"])
        for f, (rx, ry) in enumerate(rvs):
            sc.render_frame(rx, ry)
            st = sc.frame_stats()
            assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
        assert sc.launch_info()[:3] == [0, 32, 1]
        assert int((bits(sc.read_sum()) != bits(sums[depth - 1])).sum()) == 0
        sc.clear_environment()
        sc.render_frame(*rvs[0])
        assert sc.launch_info()[1] == 0
    finally:
        sc.close()
        inst.close()


# ---------------------------------------------------------------------------------------------- GPU: a furnace

FURNACE_VIEWS = (((0.0, 0.0, -3.0), 4), ((0.0, 0.0, 3.0), 5))      # (camera position on the z axis, the one face it sees: -z, +z)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", (1, 2, 4))
def test_gpu_furnace_cube_under_a_constant_sky(cr, cases, envs, rvs, depth):
    """The cube alone, E = (0.5, 1, 2) from everywhere, no lights, one frame, seen along the z axis from either side: the camera sees the
    one face whose normal is (0, 0, -1) or (0, 0, 1).  A cosine-sampled direction from a face of a convex body, started 0.0002 off it,
    cannot re-enter the body: at max_depth >= 2 every pixel's one sample is E (the primary ray missed) or albedo_face * E (it hit, bounced,
    missed); at max_depth 1 every cube pixel is exactly 0.  Tolerance 1e-6 relative: the constant map's blend makes three roundings, the
    scale and the throughput multiply one each — five half-ulps, 1.5e-7; the rest is margin.  Nothing here uses env_ref's loop.
    Why these two faces: the shader's tangent frame (integrator_ref's bu, bv: (1 + b, b, -n.x), (b, 1 + b, -n.y)) is orthonormal where
    n.x = n.y = 0 — both of its branches are, and the two views take one each — and skewed elsewhere, so that from a face with normal
    +-x or +-y some of its "cosine" directions point INTO the surface and the path re-enters the cube (by design of the reference: those
    faces are held to env_ref by bits above, where 61 of 883 such paths do)."""
    _, data, _ = cases["cube"]
    E = np.array(E_CONST, np.float64)
    for position, face in FURNACE_VIEWS:
        scene = cr.Scene(data, W, H, depth)
        try:
            scene.update(cr.Camera(position, (0.0, 0.0, 0.0), 45.0))
            set_env(scene, envs["const1"])
            scene.render_frame(*rvs[0])
            got = scene.read_sum().reshape(-1, 3).astype(np.float64)
        finally:
            scene.close()
        sky = np.abs(got - E).max(1) <= 1e-6 * E.max()
        want = np.zeros(3) if depth == 1 else FACE_ALBEDO[face].astype(np.float64) * E
        on_cube = (got == 0).all(1) if depth == 1 else (np.abs(got - want) <= 1e-6 * want).all(1)
        print(depth, position, "sky pixels", int(sky.sum()), "cube pixels", int(on_cube.sum()))
        assert (sky | on_cube).all(), got[~(sky | on_cube)][:4]
        assert sky.sum() > W * H // 4 and on_cube.sum() > W * H // 16


# ---------------------------------------------------------------------------------------------- GPU: no environment is the parent

@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "tess8", "textured"))
def test_gpu_no_environment_is_the_fused_path(cr, cornell, cornell_data, tess8, textured, envs, rvs, name):
    """before set_environment, after clear_environment and on a fresh scene: the same words and the same launch form; and a set
    environment of scale 0 gives the fused path's words through the new chain — which ties the chain to the old kernels by itself"""
    data, cam = {"cornell": (cornell_data, cornell[1]), "tess8": (tess8[1], cornell[1]), "textured": (textured[1], textured[2])}[name]
    fresh, scene = cr.Scene(data, W, H, 3), cr.Scene(data, W, H, 3)
    try:
        fresh.update(cam)
        scene.update(cam)
        fresh.render_frames(rvs)
        want, first_info = fresh.read_sum(), fresh.launch_info()
        scene.render_frames(rvs)
        assert np.array_equal(bits(scene.read_sum()), bits(want)) and scene.launch_info() == first_info
        # the fresh scene's SECOND call is the one to compare the launch form with: it has adopted the first call's tile measurement, as
        # the other scene's last call will have (frames with an environment neither start nor adopt one)
        fresh.reset()
        fresh.render_frames(rvs)
        want_info, want_stats = fresh.launch_info(), fresh.frame_stats()
        assert np.array_equal(bits(fresh.read_sum()), bits(want)) and want_info[1] & 32 == 0
        set_env(scene, envs["map16"])
        scene.reset()
        scene.render_frames(rvs)
        assert scene.launch_info()[1] == 32
        lit = scene.read_sum()
        set_env(scene, envs["zero"])
        scene.reset()
        scene.render_frames(rvs)
        assert scene.launch_info()[1] == 32
        assert int((bits(scene.read_sum()) != bits(want)).sum()) == 0
        scene.clear_environment()
        scene.reset()
        scene.render_frames(rvs)
        st = scene.frame_stats()
        assert scene.launch_info() == want_info
        assert (st["closest_rays"], st["any_rays"]) == (want_stats["closest_rays"], want_stats["any_rays"])
        assert int((bits(scene.read_sum()) != bits(want)).sum()) == 0
        print(name, "words the environment changed:", int((bits(lit) != bits(want)).sum()))
    finally:
        fresh.close()
        scene.close()


# ---------------------------------------------------------------------------------------------- GPU: feature buffers, denoiser, temporal filter

@pytest.mark.gpu
def test_gpu_aovs_do_not_depend_on_the_environment(cr, cases, envs, rvs):
    from caitlynrenderer_amd.scene import AOV_ALL
    _, data, cam = cases["cube_quad"]
    scene = cr.Scene(data, W, H, 3)
    try:
        scene.update(cam)
        out = []
        for env in (None, envs["map16"]):
            if env is not None:
                set_env(scene, env)
            scene.render_frame(*rvs[0])
            scene.render_aov(rvs[1][0], rvs[1][1], AOV_ALL)
            out.append([np.ascontiguousarray(scene.read_aov(1 << k)).tobytes() for k in range(5)])
        for k in range(5):
            assert out[0][k] == out[1][k], k
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("which", ("denoise", "temporal"))
def test_gpu_filters_on_an_environment_frame(cr, ob, cases, envs, rvs, which):
    """crt_denoise / crt_temporal are unaware of the environment: on an environment frame they give their references' bytes for that sum"""
    from caitlynrenderer_amd.scene import AOV_ALL
    _, data, cam = cases["cube_quad"]
    scene = cr.Scene(data, W, H, 3)
    try:
        scene.update(cam)
        set_env(scene, envs["map16"])
        scene.render_frames(rvs[:2])
        scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
        assert scene.launch_info()[1] == 32
        if which == "denoise":
            from test_denoise import check_denoise
            check_denoise(cr, ob, scene, 0.5, "environment frame", passes=3, demodulate=True, sigma_color=4.0, sigma_depth=0.05, normal_power_log2=7)
        else:
            from temporal_ref import view_record
            from test_temporal import check_call, directions
            _, census = check_call(cr, ob, scene, None, directions(ob, cam, W, H, rvs[0]), view_record(cam, W, H), None, None, "environment frame", 1, 32, inv=0.5)
    finally:
        scene.close()


# ---------------------------------------------------------------------------------------------- GPU: the refusals

def raw_env(texels, size=None, flags=0, rotation=None, scale=(1.0, 1.0, 1.0), reserved=(0, 0)):
    from caitlynrenderer_amd._lib import crt_environment
    e = crt_environment()
    t = None if texels is None else np.ascontiguousarray(texels, f32)
    e.texels = None if t is None else t.ctypes.data_as(C.c_void_p)
    e.size = (t.shape[0] if t is not None else 1) if size is None else size
    e.flags = flags
    e.rotation[:] = [float(x) for x in (np.eye(3, dtype=f32) if rotation is None else np.asarray(rotation, f32)).reshape(-1)]
    e.scale[:] = scale
    e.reserved[:] = reserved
    return e, t


def refusals():
    ok = np.full((2, 2, 3), 0.5, f32)
    bad_texel = [ok.copy() for _ in range(3)]
    bad_texel[0][1, 0, 2], bad_texel[1][0, 1, 0], bad_texel[2][1, 1, 1] = np.nan, np.inf, -0.25
    R = np.eye(3, dtype=f32)
    R_nan, R_inf = R.copy(), R.copy()
    R_nan[1, 2], R_inf[0, 0] = np.nan, np.inf
    return [("texels", dict(texels=None)), ("size", dict(texels=ok, size=0)), ("size", dict(texels=ok, size=4097)),
            ("texels", dict(texels=bad_texel[0])), ("texels", dict(texels=bad_texel[1])), ("texels", dict(texels=bad_texel[2])),
            ("scale", dict(texels=ok, scale=(1.0, float("nan"), 1.0))), ("scale", dict(texels=ok, scale=(float("inf"), 1.0, 1.0))),
            ("scale", dict(texels=ok, scale=(1.0, 1.0, -0.5))), ("rotation", dict(texels=ok, rotation=R_nan)), ("rotation", dict(texels=ok, rotation=R_inf)),
            ("flags", dict(texels=ok, flags=2)), ("flags", dict(texels=ok, flags=0x80000001)), ("reserved", dict(texels=ok, reserved=(0, 1))),
            ("reserved", dict(texels=ok, reserved=(7, 0)))]


@pytest.mark.gpu
@pytest.mark.parametrize("devices", (None, [0, 0]))
def test_gpu_refusals_keep_the_previous_environment(cr, cases, envs, rvs, reference, devices):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    _, data, cam = cases["cube_quad"]
    one = er.render(ir.RefScene(cases["cube_quad"][0], cam, W, H), rvs[:1], 2, envs["map16"])[0][1]
    assert L.crt_set_environment(None, None) == _lib.CRT_ERR_INVALID and b"null scene" in L.crt_last_error()
    scene = cr.Scene(data, W, H, 2)
    try:
        if devices is not None:
            scene.set_devices(devices)
        scene.update(cam)
        set_env(scene, envs["map16"])
        for field, kw in refusals():
            e, keep = raw_env(**kw)
            assert L.crt_set_environment(scene._h, C.byref(e)) == _lib.CRT_ERR_INVALID, (field, kw)
            assert field.encode() in L.crt_last_error(), (field, L.crt_last_error())
            scene.reset()
            scene.render_frame(*rvs[0])
            assert int((bits(scene.read_sum()) != bits(one)).sum()) == 0, (field, kw)          # the previous environment's words
        with pytest.raises(_lib.CrtError) as err:
            scene.set_option("accel", 1)
        assert "environment" in str(err.value)
        # the environment survives crt_reset (above) and a change does not clear the sum
        before = scene.read_sum()
        set_env(scene, envs["const1"])
        assert np.array_equal(bits(scene.read_sum()), bits(before))
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_the_bvh2_frame_mode_refuses_an_environment(cr, cases, envs, rvs):
    from caitlynrenderer_amd import _lib
    _, data, cam = cases["cube"]
    scene = cr.Scene(data, W, H, 2)
    try:
        scene.update(cam)
        scene.set_option("accel", 1)
        with pytest.raises(_lib.CrtError) as err:
            set_env(scene, envs["map16"])
        assert "accel" in str(err.value)
        scene.set_option("accel", 0)
        set_env(scene, envs["map16"])
        scene.render_frame(*rvs[0])
        assert scene.launch_info()[1] == 32
    finally:
        scene.close()
