"""The frames of instanced scenes (k_segment's instanced arms, the moved light table, the ray-class masks) held to tests/instanced_ref.py:
a numpy restatement written from include/crt.h and tests/integrator_ref.py that shares no code with oracle/ or the library (DESIGN.md
"Instanced frames as tested").

CPU cases: the reference's world_to_object and light table against the host functions by bits; the identity split of the Cornell and
textured fixtures against the flat reference by words; the conditions on the scenes (every branch of the census taken by at least 20
pixel-samples, no equal-t candidates in two instances, every ray's visibility equal to orc_trace_instances by bits); and the net's mesh:
thirteen deliberate mistakes, twelve of which must change words.  GPU cases: the HIP frame path against the reference directly — the oracle is
not involved — sums as uint32 words, ray counts against the census, the light table by bits, Scene.resolve() against resolve_ref.

All comparisons are exact."""
import types

import numpy as np
import pytest

import instanced_ref as xr
import integrator_ref as ir
from test_instances_frames import shading_of, split_mesh
from test_instances_oracle import IDENTITY, host_blas, host_scene, orc

f32 = np.float32
W, H = 44, 28               # no multiple of the 8-, 16- or 64-pixel tiles; W != H
FRAMES = 4
MAX_DEPTH = 4
MIN_BRANCH = 20
MASKS_ON = {"instance_masks": 1, "mask_primary": 0x01, "mask_bounce": 0x02, "mask_shadow": 0x04}
MASKS_SHADOW_CHANGED = {**MASKS_ON, "mask_shadow": 0x01}          # shadow rays now miss the box that primary rays miss


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- the scenes, built by hand

def rot(axis, angle):
    a = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * (K @ K)


def place(A, t):
    return np.concatenate([np.asarray(A, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(f32)


def material(albedo=(0, 0, 0), kind=0.0, emission=None, ew=-1.0, layer=-1.0):
    m = np.full(16, -1.0, f32)
    m[0:3], m[3] = albedo, kind
    m[4:7], m[7] = (0, 0, 0) if emission is None else emission, ew
    m[8:12] = 0.0
    m[12] = layer
    return m


def quad_mesh(cr, p, a, b, mtl, normal=None, flat=None, uv=False, mats=None, fourth=1.0):
    """the quad p, p + a, p + a + b, p + fourth b as two triangles (materials mtl[0], mtl[1]); vertex normals `normal`, or the flat integer
    normal `flat` (vn.w == 0); uv: a scale for texcoords that leave [0, 1], or False for none"""
    p, a, b = (np.asarray(x, f32) for x in (p, a, b))
    v = np.array([p, p + a, p + a + b, p + f32(fourth) * b], f32)
    vn = [0, 0, 0, 1] if flat is None else list(flat) + [0]
    t = np.array([[0, 1, 2, mtl[0]] + vn + ([0, 1, 2, 0] if uv else [-1, -1, -1, 0]),
                  [0, 2, 3, mtl[1]] + vn + ([0, 2, 3, 0] if uv else [-1, -1, -1, 0])], np.int32)
    n = np.zeros((0, 3), f32) if flat is not None else np.array([normal], f32)
    tc = (np.array([[-0.3, 0.1], [1.6, 0.1], [1.6, 2.2], [-0.3, 2.2]], f32) * f32(uv)).astype(f32) if uv else np.zeros((0, 2), f32)
    return cr.Mesh(v, n, tc, t, mats, np.zeros((0, 18), f32))


def box_mesh(cr, mtl, mats):
    """the box [-0.5, 0.5] x [0, 1] x [-0.5, 0.5]: 12 triangles, one outward vertex normal per face"""
    lo, hi = np.array([-0.5, 0.0, -0.5]), np.array([0.5, 1.0, 0.5])
    v, n, t = [], [], []
    for axis in range(3):
        for side in (0, 1):
            a, b = (axis + 1) % 3, (axis + 2) % 3
            c = [np.zeros(3) for _ in range(4)]
            for k, (sa, sb) in enumerate(((0, 0), (1, 0), (1, 1), (0, 1))):
                c[k][axis] = (hi if side else lo)[axis]
                c[k][a] = (hi if sa else lo)[a]
                c[k][b] = (hi if sb else lo)[b]
            i, f = len(v), len(n)
            v += c
            nn = np.zeros(3)
            nn[axis] = 1.0 if side else -1.0
            n.append(nn)
            t += [[i, i + 1, i + 2, mtl, f, f, f, 1, -1, -1, -1, 0], [i, i + 2, i + 3, mtl, f, f, f, 1, -1, -1, -1, 0]]
    return cr.Mesh(np.array(v, f32), np.array(n, f32), np.zeros((0, 2), f32), np.array(t, np.int32), mats, np.zeros((0, 18), f32))


def quad_lights(mesh, normal, emission):
    """one light per triangle of a quad mesh: p = v0, u = v1 - v0, v = v2 - v0, area = |u x v| as the loader has it; the pdf words are
    deliberately wrong (7): the table must not depend on them"""
    out = []
    for t in mesh.triangles:
        p, q, r = (mesh.vertices[t[k]] for k in range(3))
        u, v = q - p, r - p
        area = float(np.linalg.norm(np.cross(u.astype(np.float64), v.astype(np.float64))))
        out.append(np.concatenate([p, u, v, normal, emission, [area, 7.0, 0.0]]))
    return np.array(out, f32)


# materials of the yard.  0 - 6 are the meshes' own; 7 - 9 are reached through a material offset only
M_FLOOR, M_BOX, M_PANEL, M_LAMP0, M_LAMP1, M_WALL, M_BULB, M_MIRROR, M_TEXTURED, M_BULB_CLAMPED = range(10)
LAMP_E, WALL_E, BULB_E = (9.0, 8.0, 7.0), (3.0, 3.5, 4.5), (5.0, 2.5, 1.5)


def yard_materials():
    return np.array([material((0.6, 0.6, 0.6)), material((0.8, 0.5, 0.3)), material((0.3, 0.7, 0.4)),
                     material(emission=LAMP_E, ew=0.0), material(emission=LAMP_E, ew=1.0), material(emission=WALL_E, ew=0.0),
                     material(emission=BULB_E, ew=0.0), material((0.9, 0.9, 0.9), kind=1.0), material((0.5, 0.5, 0.5), layer=1.0),
                     material(emission=BULB_E, ew=1.0)], f32)


def yard(cr, textures, moved=False):
    """Scene (Y), or (Y') with moved=True: -> a namespace of everything the reference and the handle take.
    meshes: 0 floor (flat integer normal; its unused texcoords give the panel's a base other than 0), 1 box, 2 panel (vertex normals of length 2, texcoords), 3 lamp (two lights, a quad that is no
    parallelogram so that their areas differ), 4 wall (light-less; the static light's emissive quad), 5 bulb (one light)."""
    mats = yard_materials()
    meshes = [quad_mesh(cr, (-5, 0, -4), (0, 0, 10), (10, 0, 0), (M_FLOOR, M_FLOOR), flat=(0, 1, 0), uv=0.37, mats=mats),
              box_mesh(cr, M_BOX, mats),
              quad_mesh(cr, (-1, 0, 0), (2, 0, 0), (0, 1.5, 0), (M_PANEL, M_PANEL), normal=(0, 0, -2), uv=True, mats=mats),
              quad_mesh(cr, (-1.5, 2.2, -0.6), (0, 0, 2.2), (3.0, 0, 0), (M_LAMP0, M_LAMP1), normal=(0, -1, 0), mats=mats, fourth=0.6),
              quad_mesh(cr, (4.7, 0.3, 0.0), (0, 0, 3.0), (0, 2.0, 0), (M_WALL, M_WALL), normal=(-1, 0, 0), mats=mats),
              quad_mesh(cr, (-0.5, 0, 0), (1, 0, 0), (0, 1, 0), (M_BULB, M_BULB), normal=(0, 0, -1), mats=mats)]
    lamp_lights = quad_lights(meshes[3], (0, -1, 0), LAMP_E)
    bulb_lights = quad_lights(meshes[5], (0, 0, -1), BULB_E)[:1]
    bulb_lights[0, 6:9] = meshes[5].vertices[3] - meshes[5].vertices[0]          # one light over the whole quad: u, v its edges
    bulb_lights[0, 15] = 1.0
    static = quad_lights(meshes[4], (-1, 0, 0), WALL_E)[:1]
    static[0, 6:9] = meshes[4].vertices[3] - meshes[4].vertices[0]
    static[0, 15] = 6.0
    numerically_identity = IDENTITY.copy()
    numerically_identity[1, 0] = numerically_identity[0, 2] = -0.0
    numerically_identity[:, 3] = (-2.2, 0.05, 0.3)
    shear = np.array([[1, 0.4, 0], [0, 1, 0], [0.2, 0, 1]])
    # (matrix, mesh, mask, material offset); masks: bit 0 primary, bit 1 bounce, bit 2 shadow, so 0xfe hides from primary rays, ...
    inst = [(place(np.eye(3) * 1.25, (0.3, -0.03, 0.4)), 0, 0xff, 0),
            (IDENTITY, 1, 0xff, 0),
            (numerically_identity, 1, 0xff, 0),
            (place(rot((0, 1, 0), 0.5) @ np.diag([1.4, 1.7, 1.0]), (2.1, 0.04, 0.9)), 1, 0xfb, 0),           # hidden from shadow rays
            (place(rot((0, 1, 0), -0.3) @ np.diag([-1.2, 1.0, 1.0]), (-1.0, 0.06, 2.4)), 1, 0xff, 0),        # a mirror
            (place(shear, (1.0, 0.02, 2.8)), 1, 0xfe, 0),                                                    # hidden from primary rays
            (place(rot((0, 1, 0), 0.8) * 1.3, (-3.3, 0.03, 1.6)), 1, 0xff, M_MIRROR - M_BOX),
            (place(rot((0, 1, 0), 0.4) @ np.diag([1.3, 0.9, 1.0]), (3.0, 0.1, 4.6)), 2, 0xff, 0),
            (place(rot((0, 1, 0), -0.35) * 1.1, (-2.8, 0.12, 4.9)), 2, 0xff, M_TEXTURED - M_PANEL),
            (place(rot((0, 0, 1), 0.35) @ rot((0, 1, 0), 0.4), (-1.5, -0.2, 1.0)), 3, 0xff, 0),
            (place(rot((0, 0, 1), -0.3) @ np.diag([1.0, 1.0, -1.3]), (1.6, -0.3, 2.6)), 3, 0xff, 0),          # a mirrored lamp
            (IDENTITY, 3, 0xfd, 0),                                                                          # a lamp hidden from bounce rays
            (IDENTITY, 4, 0xff, 0),
            (place(rot((1, 0, 0), -0.8) @ np.diag([2.9, 2.6, 1.5]), (-0.9, 0.15, 3.9)), 5, 0xff, M_BULB_CLAMPED - M_BULB),   # ew = 1 >= nl = 1
            (place(rot((0, 1, 0), 0.2) * 1.5, (0.4, 1.3, 5.6)), 5, 0xff, 0),
            # a mirror lying under the boxes and the lamps: box sides -> mirror -> lamp is the path on which a Mirror hit must set is_specular
            (place(rot((1, 0, 0), np.pi / 2) @ np.diag([2.6, 1.9, 1.0]), (0.2, 0.01, -0.3)), 2, 0xff, M_MIRROR - M_PANEL)]
    if moved:
        rng = np.random.default_rng(2601)
        new = []
        for k, (m, mesh, mask, off) in enumerate(inst):
            m = m.astype(np.float64)
            if mesh in (0, 4):
                m[:, 3] += (0.05, -0.02, 0.1)                                        # the floor and the wall slide a little (the wall's light is static)
            else:
                m[:, :3] = rot((0, 1, 0), rng.uniform(-0.4, 0.4)) @ m[:, :3] * rng.uniform(0.9, 1.15)
                m[:, 3] += rng.uniform(-0.35, 0.35, 3) * (1, 0.3, 1) + (0, 0.2, 0)
            if k == 9:                                                                # one lamp turned over, about its own centre c
                c, R = np.array([0.0, 2.2, 0.5]), rot((0, 0, 1), np.pi)
                m[:, 3] += m[:, :3] @ (c - R @ c)
                m[:, :3] = m[:, :3] @ R
            new.append((m.astype(f32), mesh, (0xfe, 0xfd, 0xfb, 0xff)[(k + 1) % 4] if k not in (0, 12) else 0xff, off))
        inst = new
    cam = cr.Camera((0.4, 3.6, -8.4), (0.0, 1.1, 1.2), 50.0)
    return types.SimpleNamespace(meshes=meshes, M=np.array([i[0] for i in inst], f32), mesh_of=np.array([i[1] for i in inst]),
                                 masks=np.array([i[2] for i in inst], np.uint32), offsets=np.array([i[3] for i in inst], np.uint32),
                                 mats=mats, static=static, mesh_lights=[None, None, None, lamp_lights, None, bulb_lights], textures=textures, cam=cam)


def empty_table_scene(cr):
    """Scene (E): a floor, an emissive panel on a light-less mesh — reached through a material offset, because create refuses an emissive
    material of a light-less mesh's OWN triangles whose ew >= n_static (= 0 here) — and a lamp mesh with one light and no instance: a
    scene with mesh lights whose table is empty."""
    mats = np.array([material((0.7, 0.7, 0.7)), material((0.2, 0.2, 0.2)), material(emission=(2.0, 3.0, 4.0), ew=0.0),
                     material(emission=(1.0, 1.0, 1.0), ew=0.0)], f32)
    meshes = [quad_mesh(cr, (-5, 0, -4), (0, 0, 10), (10, 0, 0), (0, 0), flat=(0, 1, 0), mats=mats),
              quad_mesh(cr, (-2, 0, 0), (4, 0, 0), (0, 2.5, 0), (1, 1), normal=(0, 0, -1), mats=mats),
              quad_mesh(cr, (-0.5, 0, 0), (1, 0, 0), (0, 1, 0), (3, 3), normal=(0, 0, -1), mats=mats)]
    lamp = quad_lights(meshes[2], (0, 0, -1), (1.0, 1.0, 1.0))[:1]
    M = np.array([place(np.eye(3) * 1.25, (0.3, -0.03, 0.4)), place(rot((0, 1, 0), 0.3) @ np.diag([1.2, 1.0, 1.0]), (0.2, 0.3, 3.0))], f32)
    return types.SimpleNamespace(meshes=meshes, M=M, mesh_of=np.array([0, 1]), masks=np.array([0xff, 0xff], np.uint32),
                                 offsets=np.array([0, 1], np.uint32), mats=mats, static=np.zeros((0, 18), f32), mesh_lights=[None, None, lamp],
                                 textures=None, cam=cr.Camera((0.4, 3.6, -8.4), (0.0, 1.1, 1.2), 50.0))


def identity_split(cr, mesh, cam, parts):
    meshes, _ = split_mesh(cr, mesh, parts)
    return types.SimpleNamespace(meshes=meshes, M=np.array([IDENTITY] * parts, f32), mesh_of=np.arange(parts), masks=np.full(parts, 0xff, np.uint32),
                                 offsets=np.zeros(parts, np.uint32), mats=mesh.materials, static=mesh.lights, mesh_lights=None,
                                 textures=getattr(mesh, "albedo_textures", None), cam=cam)


def reordered(s, order):
    return types.SimpleNamespace(**{**vars(s), "M": s.M[order], "mesh_of": s.mesh_of[order], "masks": s.masks[order], "offsets": s.offsets[order]})


REORDER = np.array([11, 3, 14, 0, 9, 6, 1, 13, 15, 4, 10, 2, 12, 8, 5, 7])
NEW_LAMP_LIGHTS_SCALE = f32(0.8)


def with_new_lamp_lights(s):
    """the lamp mesh's object lights after crt_scene_set_mesh_lights: shrunk towards p and dimmer, so that table and picture both change"""
    l = s.mesh_lights[3].copy()
    l[:, 3:9] = (l[:, 3:9] * NEW_LAMP_LIGHTS_SCALE).astype(f32)
    l[:, 12:15] = (l[:, 12:15] * f32(0.5)).astype(f32)
    l[:, 15] = np.linalg.norm(np.cross(l[:, 3:6].astype(np.float64), l[:, 6:9].astype(np.float64)), axis=1)
    ml = list(s.mesh_lights)
    ml[3] = l
    return types.SimpleNamespace(**{**vars(s), "mesh_lights": ml})


def ref_scene(s, options=None, **kw):
    return xr.InstancedRef(s.meshes, s.M, s.mesh_of, s.masks, s.offsets, s.mats, s.static, s.mesh_lights, s.textures, s.cam, W, H, options=options, **kw)


# ---------------------------------------------------------------------------------------------- shared, computed once

@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def scenes(cr, cornell, textured):
    tex = textured[0].albedo_textures
    y = yard(cr, tex)
    return {"Y": y, "Y'": yard(cr, tex, moved=True), "E": empty_table_scene(cr), "Y_reordered": reordered(y, REORDER),
            "Y_new_lamp_lights": with_new_lamp_lights(y),
            "I_cornell": identity_split(cr, cornell[0], cornell[1], 4), "I_textured": identity_split(cr, textured[0], textured[2], 5)}


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make(key)
        return self[key]


OPTIONS = {"off": None, "on": MASKS_ON, "shadow_changed": MASKS_SHADOW_CHANGED}
# every (scene, masks) whose reference run a GPU case compares with
REFERENCE_RUNS = (("I_cornell", "off"), ("I_textured", "off"), ("Y", "off"), ("Y", "on"), ("Y", "shadow_changed"), ("E", "off"),
                  ("Y_reordered", "off"), ("Y'", "on"), ("Y_new_lamp_lights", "off"))


@pytest.fixture(scope="module")
def reference(scenes, rvs):
    """(scene name, masks) -> (sums[depth - 1], per-frame census [frame][depth - 1], census[depth - 1] over the 4 frames, the scene with its
    logged rays): one run at MAX_DEPTH gives every shorter depth"""
    def make(key):
        name, masks = key
        scene = ref_scene(scenes[name], OPTIONS[masks], log=True)
        sums, _, total, per_frame = ir.render(scene, rvs, MAX_DEPTH)
        for s in sums:
            s.setflags(write=False)
        return sums, per_frame, total, scene
    return _Lazy(make)


# ---------------------------------------------------------------------------------------------- the reference's own arithmetic

ALL_SCENES = ("Y", "Y'", "E", "Y_reordered", "I_cornell")


@pytest.mark.parametrize("name", ALL_SCENES)
def test_world_to_object_equals_the_host_function(cr, scenes, name):
    for m in scenes[name].M:
        assert np.array_equal(bits(xr.world_to_object(m)).reshape(12), bits(cr.instance_inverse(m))), m


def host_table(cr, s):
    parts = [np.asarray(s.static, f32).reshape(-1, 18)]
    for m, mesh in zip(s.M, s.mesh_of):
        if s.mesh_lights[mesh] is not None:
            parts.append(cr.instance_lights(m, s.mesh_lights[mesh]))
    return cr.lights_finish(np.concatenate(parts))


@pytest.mark.parametrize("name", ("Y", "Y'", "E", "Y_reordered", "Y_new_lamp_lights"))
def test_light_table_equals_the_host_functions(cr, scenes, name):
    s = scenes[name]
    ref = ref_scene(s)
    want = host_table(cr, s)
    assert ref.lights.shape == want.shape and np.array_equal(bits(ref.lights), bits(want))
    if name != "E":
        assert ref.lights.shape[0] == 1 + 3 * 2 + 2 and (ref.lights[:, 16] != 7.0).all()
        # the mirrored lamp's lights keep facing the way its shading normal faces: down
        k = int(np.nonzero(ref.mirrored & (ref.mesh_of == 3))[0][0])
        assert (ref.lights[ref.first[k]:ref.first[k] + 2, 10] < -0.8).all()
    else:
        assert ref.lights.shape[0] == 0


@pytest.mark.parametrize("name,flat", (("I_cornell", "cornell"), ("I_textured", "textured")))
def test_identity_split_equals_the_flat_reference(cornell, textured, scenes, reference, rvs, name, flat):
    """(I): the instanced reference gives the flat reference's words at every depth, and its counts"""
    mesh, cam = (cornell[0], cornell[1]) if flat == "cornell" else (textured[0], textured[2])
    want, _, total, _ = ir.render(ir.RefScene(mesh, cam, W, H), rvs, MAX_DEPTH)
    sums, _, census, scene = reference[(name, "off")]
    assert scene.flag.all()
    for depth in range(MAX_DEPTH):
        assert int((bits(sums[depth]) != bits(want[depth])).sum()) == 0, depth
        for key in ir.CENSUS_KEYS:
            assert census[depth][key] == total[depth][key], (depth, key)
    assert sums[2].max() > 0.4


# ---------------------------------------------------------------------------------------------- the conditions on the scenes

UNMASKED_KEYS = tuple(f"hits_{kind}_{c}" for kind in ("identity", "general", "mirrored") for c in ("primary", "bounce")) + (
    "hits_with_offset", "textured_through_offset", "mirror_on_general", "emitter_after_bounce_clamped", "emitter_after_bounce_unclamped",
    "emitter_after_bounce_lightless_mesh", "nee_moved_light", "nee_mirrored_lamp_light", "flat_normal_hit", "non_unit_normal_hit",
    "shadow_occluded", "shadow_clear", "miss_first", "miss_later", "emitter_direct",
    "emitter_through_mirror_after_bounce")
MASKED_KEYS = ("mask_changes_primary", "mask_changes_bounce", "shadow_blocked_only_by_hidden")


def test_every_branch_is_taken(reference):
    """the census in the reference alone, paths of 4 segments, 4 frames: no rule is tested emptily"""
    y = reference[("Y", "off")][2][MAX_DEPTH - 1]
    for key in UNMASKED_KEYS:
        assert y[key] >= MIN_BRANCH, (key, y)
    ym = reference[("Y", "on")][2][MAX_DEPTH - 1]
    for key in MASKED_KEYS:
        assert ym[key] >= MIN_BRANCH, (key, ym)
    # mask_shadow alone changed: another box stops casting its shadow, and the picture is another one
    assert reference[("Y", "shadow_changed")][2][2]["shadow_blocked_only_by_hidden"] > 0
    assert int((bits(reference[("Y", "shadow_changed")][0][2]) != bits(reference[("Y", "on")][0][2])).sum()) > 100
    e = reference[("E", "off")][2][MAX_DEPTH - 1]
    assert e["emitter_empty_table"] >= MIN_BRANCH and e["emitter_direct"] >= MIN_BRANCH and e["shadow_rays"] == 0, e


def test_no_ray_has_equal_t_candidates_in_two_instances(reference):
    """every reference run that a GPU case compares with, computed here if no earlier test has: zero path or shadow rays whose best two
    candidate hits lie in different instances at equal t (the oracle comparison below cannot see such a tie: both sides give it to the
    lower instance)"""
    assert {(n, m) for n, m, _ in GPU_CASES} | {("Y_reordered", "off"), ("Y'", "on"), ("Y_new_lamp_lights", "off")} == set(REFERENCE_RUNS)
    for key in REFERENCE_RUNS:
        for depth in range(MAX_DEPTH):
            assert reference[key][2][depth]["cross_instance_ties"] == 0, (key, depth)


def test_no_nonemitter_has_a_zero_normal(scenes):
    for name in ("Y", "E"):
        for m in scenes[name].meshes:
            assert (np.abs(m.normals).max(1) > 0).all() and (m.triangles[m.triangles[:, 7] == 0][:, 4:7] != 0).any(1).all()


def grazing_margin(s):
    """per instance the two sides of crt_instances_trace's bound cond_inf(A) (2 |o|_inf + B + |t|_inf) <= 51 B, o the camera (every later
    origin lies on the scene, nearer the origin)"""
    c = s.cam.c if hasattr(s.cam, "c") else s.cam
    o = float(np.abs(np.asarray(c.position[:], np.float64)).max())
    out = []
    for m, mesh in zip(s.M.astype(np.float64), s.mesh_of):
        A, t = m[:, :3], m[:, 3]
        V = s.meshes[mesh].vertices.astype(np.float64) @ A.T + t
        B = float(np.abs(V).max())
        cond = float(np.linalg.norm(A, np.inf) * np.linalg.norm(np.linalg.inv(A), np.inf))
        out.append((cond * (2 * o + B + float(np.abs(t).max())), 51 * B, cond))
    return out


@pytest.mark.parametrize("name", ("Y", "Y'", "E"))
def test_grazing_margin_bound_holds_by_a_wide_margin(scenes, name):
    sides = grazing_margin(scenes[name])
    worst = max(sides, key=lambda x: x[0] / x[1])
    print(name, "worst instance: cond %.2f, %.1f <= %.1f" % (worst[2], worst[0], worst[1]))
    assert all(c < 4.0 and lhs <= 0.5 * rhs for lhs, rhs, c in sides), sides


@pytest.mark.parametrize("name,masks", REFERENCE_RUNS)
def test_visibility_equals_the_two_level_oracle(cr, ob, scenes, reference, name, masks):
    """every closest ray and every shadow ray of the reference's own frames through orc_trace_instances on arrays assembled on the host:
    t, u, v, id, instance and occlusion by bits, so that neither exception of the contract (equal t, grazing margin) occurs on these
    inputs"""
    s = scenes[name]
    scene = reference[(name, masks)][3]
    host = host_scene(cr, [host_blas(cr, m) for m in s.meshes], list(s.M), list(s.mesh_of), s.masks)
    n_closest = n_shadow = 0
    for log in scene.rays:
        rays = np.zeros(log["o"].shape[0], cr.RAY_DT)
        rays["o"], rays["d"], rays["tmax"] = log["o"], log["d"], log["tmax"]
        rays["pad"] = scene.class_mask[log["ray_class"]]
        if log["ray_class"] == 2:
            hits, ids, _, _, refused = orc(ob, host, rays, ob.ANY, masked=scene.masked)
            assert np.array_equal(hits["tri"] >= 0, log["tri"] >= 0)
            n_shadow += rays.shape[0]
        else:
            hits, ids, _, _, refused = orc(ob, host, rays, ob.CLOSEST, masked=scene.masked)
            hit = log["tri"] >= 0
            assert np.array_equal(ids, log["instance"]) and np.array_equal(hits["tri"], log["tri"])
            for k in ("t", "u", "v"):
                assert np.array_equal(bits(hits[k][hit]), bits(log[k][hit])), k
            n_closest += rays.shape[0]
        assert refused.sum() == 0
    total = reference[(name, masks)][2][MAX_DEPTH - 1]
    assert (n_closest, n_shadow) == (total["closest_rays"], total["shadow_rays"]) and n_closest > FRAMES * W * H


# ---------------------------------------------------------------------------------------------- the net's mesh

# break -> the scenes (name, masks) on one of which it must change words at some depth (DESIGN.md has the whole table)
BOTH_YARDS = (("Y", "off"), ("Y'", "on"))
SENSITIVE = {"light_normal_by_A": BOTH_YARDS, "shadow_mask_bounce": (("Y", "on"), ("Y'", "on")), "bounce_mask_primary": (("Y", "on"), ("Y'", "on")),
             "clamp_nl": BOTH_YARDS, "first_in_other_order": BOTH_YARDS, "unit_normal": BOTH_YARDS, "hit_point_object_ray": BOTH_YARDS,
             "vt_without_base": BOTH_YARDS, "lightless_uses_first": BOTH_YARDS, "empty_table_prev_pdf": (("E", "off"),), "pdf_as_given": BOTH_YARDS,
             "mirror_keeps_is_specular": BOTH_YARDS}


def differing_words(scenes, reference, rvs, name, masks, brk):
    scene = ref_scene(scenes[name], OPTIONS[masks], breaks=(brk,), first_order=REORDER if name != "E" else None)
    sums = ir.render(scene, rvs, MAX_DEPTH)[0]
    return [int((bits(a) != bits(b)).sum()) for a, b in zip(sums, reference[(name, masks)][0])]


@pytest.mark.parametrize("brk", sorted(SENSITIVE))
def test_a_broken_rule_changes_words(scenes, reference, rvs, brk):
    total = 0
    for name, masks in SENSITIVE[brk]:
        diff = differing_words(scenes, reference, rvs, name, masks, brk)
        print(brk, name, masks, "differing words at depths 1-4:", diff)
        total += sum(diff)
    assert total > 0, brk


def test_ties_to_the_higher_instance_change_nothing(scenes, reference, rvs):
    """break 12: no two instances of (Y) share a plane, so the tie rule is not what these scenes test (tests/test_instances_oracle.py's
    coincident instances hold it)"""
    assert max(differing_words(scenes, reference, rvs, "Y", "off", "ties_to_higher_instance")) == 0


# ---------------------------------------------------------------------------------------------- the GPU against the reference

def open_scene(cr, s, depth, builder="sah", options=None):
    inst = cr.InstancedScene(s.meshes, cr.instances_array(s.M, s.mesh_of, masks=s.masks, material_offsets=s.offsets), builder=builder)
    sc = inst.frame_scene(shading_of(s.meshes), s.mats, s.static, W, H, depth, textures=s.textures, mesh_lights=s.mesh_lights)
    sc.update(s.cam)
    for k, v in (options or {}).items():
        sc.set_option(k, v)
    if options:
        sc.reset()
    return inst, sc


def render_and_check(sc, entry, rvs, depth, one_call=False):
    sums, per_frame, total, _ = entry
    if one_call:
        sc.render_frames(rvs)                       # an instanced scene queues the frames one by one (several samples per launch are not
        st = sc.frame_stats()                       # offered), and crt_get_frame_stats describes the last launch: the last frame
        assert (st["closest_rays"], st["any_rays"]) == (per_frame[-1][depth - 1]["closest_rays"], per_frame[-1][depth - 1]["shadow_rays"])
    else:
        for f, (rx, ry) in enumerate(rvs):
            sc.render_frame(rx, ry)
            st = sc.frame_stats()
            assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
    assert st["stack_overflows"] == 0
    got = sc.read_sum()
    bad = np.nonzero((bits(got) != bits(sums[depth - 1])).any(-1))
    assert bad[0].size == 0, (bad[0].size, list(zip(*bad))[:4], got[bad][:3], sums[depth - 1][bad][:3])
    sc.frame_count = len(rvs)
    rgba = sc.resolve()
    assert np.array_equal(rgba, ir.resolve_ref(got, f32(1.0 / len(rvs))))


def close(inst, sc):
    sc.close()
    inst.close()


GPU_CASES = [("I_cornell", "off", 1), ("I_cornell", "off", 3), ("I_textured", "off", 1), ("I_textured", "off", 3),
             ("Y", "off", 1), ("Y", "off", 2), ("Y", "off", 3), ("Y", "off", 4), ("Y", "on", 3), ("Y", "shadow_changed", 3),
             ("E", "off", 1), ("E", "off", 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,masks,depth", GPU_CASES)
def test_gpu_frames_equal_the_reference(cr, scenes, reference, rvs, name, masks, depth):
    """the sums after four render_frame calls as uint32 words, each frame's closest and shadow ray counts against the census, the light
    table by bits and the resolved bytes against resolve_ref.  "shadow_changed": rendered with MASKS_ON first, then mask_shadow alone is
    changed and crt_reset follows, as the header says."""
    first = MASKS_ON if masks == "shadow_changed" else OPTIONS[masks]
    inst, sc = open_scene(cr, scenes[name], depth, options=first)
    try:
        if masks == "shadow_changed":
            sc.render_frame(*rvs[0])
            sc.set_option("mask_shadow", MASKS_SHADOW_CHANGED["mask_shadow"])
            sc.reset()
        if scenes[name].mesh_lights is not None:
            assert np.array_equal(bits(cr.read_lights(sc)), bits(reference[(name, masks)][3].lights))
        render_and_check(sc, reference[(name, masks)], rvs, depth)
    finally:
        close(inst, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("render_frames", "lbvh", "reordered"))
def test_gpu_variants_equal_the_reference(cr, scenes, reference, rvs, variant):
    """(Y), paths of 3 segments, once through each other way to the same frame; "reordered": the same instances given in another order
    against the reference run with that order (the instance index is part of the tie rule and of first[])"""
    name = "Y_reordered" if variant == "reordered" else "Y"
    inst, sc = open_scene(cr, scenes[name], 3, builder="lbvh" if variant == "lbvh" else "sah")
    try:
        assert np.array_equal(bits(cr.read_lights(sc)), bits(reference[(name, "off")][3].lights))
        render_and_check(sc, reference[(name, "off")], rvs, 3, one_call=variant == "render_frames")
    finally:
        close(inst, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("way", ("refit", "set", "set_mesh_lights"))
def test_gpu_moved_yard_equals_the_reference(cr, scenes, reference, rvs, way):
    """(Y) -> (Y'), masks on, paths of 3 segments: a frame of (Y), then the move, crt_reset, and four frames against the reference of
    the moved scene; the light table by bits before and after"""
    y = scenes["Y"]
    target, masks = ("Y_new_lamp_lights", "off") if way == "set_mesh_lights" else ("Y'", "on")
    inst, sc = open_scene(cr, y, 3, options=OPTIONS[masks])
    try:
        assert np.array_equal(bits(cr.read_lights(sc)), bits(reference[("Y", masks)][3].lights))
        sc.render_frame(*rvs[0])
        s = scenes[target]
        if way == "set_mesh_lights":
            cr.set_mesh_lights(sc, 3, s.mesh_lights[3])
        else:
            rec = cr.instances_array(s.M, s.mesh_of, masks=s.masks, material_offsets=s.offsets)
            inst.refit(rec) if way == "refit" else inst.set(rec)
        sc.reset()
        assert np.array_equal(bits(cr.read_lights(sc)), bits(reference[(target, masks)][3].lights))
        render_and_check(sc, reference[(target, masks)], rvs, 3)
    finally:
        close(inst, sc)
