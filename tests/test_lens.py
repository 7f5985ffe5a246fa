"""The thin-lens camera (crt_camera's aperture and focal_dist) held to tests/lens_ref.py: the contract of include/crt.h
restated in float32 numpy over integrator_ref's and instanced_ref's own loops.  The C oracle has no lens.

CPU cases: the reference at aperture 0 is integrator_ref.primary_rays by bits; Camera.set_lens round-trips through crt_camera; every ray
of four frames passes, in float64, through the pinhole ray's point of the plane of focus; the lens points lie on the disc, in all four
quadrants; a lens frame differs from the pinhole frame.  GPU cases: the primary rays out of k_raygen_lens as a multiset of 28-byte rows,
frames as uint32 words with their ray counts and resolved bytes, every other way to the same frame, the way back to the pinhole, the
AOVs' independence of the aperture, instanced scenes, and crt_set_camera's refusals.

All comparisons of frames and rays are exact.  The bounds of the focus and lens tests are derived where they stand."""
import ctypes as C
import types

import numpy as np
import pytest

import integrator_ref as ir
import lens_ref as lr
from test_instanced_ref import box_mesh, material, place, quad_lights, quad_mesh, rot
from test_instances_frames import shading_of
from test_integrator_ref import hand_made_mesh

f32 = np.float32
W, H = 44, 28               # conftest's small frame: no multiple of the 8-, 16- or 64-pixel tiles; W != H
FRAMES = 4
MAX_DEPTH = 4
HAND_MODEST = (0.03, 1.5)   # (aperture, focal_dist) on the hand-made scene
HOSTILE = (0.5, 0.5)        # a lens as wide as its plane of focus is far


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def diagonal(mesh):
    v = np.asarray(mesh.vertices, np.float64).reshape(-1, 3)
    return float(np.linalg.norm(v.max(0) - v.min(0)))


# ---------------------------------------------------------------------------------------------- shared, computed once

@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def cases(cr, cornell, cornell_data, tess8, textured):
    """name -> (mesh, SceneData, camera), test_integrator_ref's scenes rebuilt"""
    out = {"cornell": (cornell[0], cornell_data, cornell[1]), "tess8": (tess8[0], tess8[1], cornell[1]),
           "textured": (textured[0], textured[1], textured[2])}
    for name, kw in (("hand", {}), ("hand_unlit", {"lit": False}), ("hand_lambert", {"mirror": False})):
        mesh, cam = hand_made_mesh(cr, **kw)
        out[name] = (mesh, cr.SceneData.build(mesh, cam), cam)
    return out


@pytest.fixture(scope="module")
def settings(cases):
    """(scene, "modest" | "hostile") -> (aperture, focal_dist) as float32.  Modest: 0.03 / 1.5 on the hand-made scenes, and the same ratio
    to the diagonal of the vertices' bounds on the Cornell-based ones."""
    hand = diagonal(cases["hand"][0])
    out = {}
    for name, (mesh, _, _) in cases.items():
        k = 1.0 if name.startswith("hand") else diagonal(mesh) / hand
        out[(name, "modest")] = (f32(HAND_MODEST[0] * k), f32(HAND_MODEST[1] * k))
        out[(name, "hostile")] = (f32(HOSTILE[0]), f32(HOSTILE[1]))
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


@pytest.fixture(scope="module")
def reference(cases, settings, rvs):
    """(scene, "modest" | "hostile" | "pinhole" | "modest_nojitter") -> (sums[depth - 1], per-frame census [frame][depth - 1], census over
    the 4 frames): one run at MAX_DEPTH gives every shorter depth"""
    def make(key):
        name, lens = key
        mesh, _, cam = cases[name]
        scene = ir.RefScene(mesh, cam, W, H)
        if lens == "pinhole":
            sums, _, total, per_frame = ir.render(scene, rvs, MAX_DEPTH)
        else:
            a, fd = settings[(name, lens.replace("_nojitter", ""))]
            sums, _, total, per_frame = lr.render(scene, rvs, MAX_DEPTH, a, fd, jitter=not lens.endswith("_nojitter"))
        return _frozen(sums), per_frame, total
    return _Lazy(make)


def lens_camera(cr, cam, aperture, focal_dist):
    """a copy of `cam` (a Camera or conftest's _Cam) with the lens set"""
    from caitlynrenderer_amd._lib import crt_camera
    c = crt_camera()
    C.memmove(C.byref(c), C.byref(cam.c), C.sizeof(crt_camera))
    c.aperture, c.focal_dist = float(aperture), float(focal_dist)
    return types.SimpleNamespace(c=c)


# ---------------------------------------------------------------------------------------------- CPU: the reference and the contract

@pytest.mark.parametrize("name", ("cornell", "hand"))
def test_aperture_zero_is_the_pinhole_reference(cases, rvs, name):
    mesh, _, cam = cases[name]
    scene = ir.RefScene(mesh, cam, W, H)
    for jitter in (True, False):
        for rx, ry in rvs:
            o, d, rng, census = ir.primary_rays(scene, rx, ry, jitter=jitter)
            got = lr.lens_rays(scene, rx, ry, 0.0, float("nan"), jitter=jitter)
            assert np.array_equal(bits(got["o"]), bits(o)) and np.array_equal(bits(got["d"]), bits(d))
            assert np.array_equal(bits(got["rng"].sx), bits(rng.sx)) and np.array_equal(bits(got["rng"].sy), bits(rng.sy))
            assert got["census"] == census
            # and the restated view vector is the pinhole's: normalize(v) gives its directions
            v, rng_v, _ = lr.view_vectors(scene, rx, ry, jitter)
            assert np.array_equal(bits(ir.normalize(v)), bits(d)) and np.array_equal(bits(rng_v.sx), bits(rng.sx))


def test_set_lens_round_trips_through_crt_camera(cr):
    cam = cr.Camera((0.0, 0.5, 0.0), (0.0, 0.5, 1.0), 60.0)
    assert cam.aperture == 0.0 and cam.focal_dist == float(f32(0.1))          # Camera.h's defaults
    before = bytes(cam.c)[:13 * 4]
    assert cam.set_lens(0.03, 1.5) is cam
    assert (cam.c.aperture, cam.c.focal_dist) == (float(f32(0.03)), 1.5)
    assert (cam.aperture, cam.focal_dist) == (float(f32(0.03)), 1.5)
    assert bytes(cam.c)[:13 * 4] == before                                    # position, basis and fov untouched
    cam.set_lens(0, 7)
    assert (cam.c.aperture, cam.c.focal_dist) == (0.0, 7.0)


@pytest.mark.parametrize("lens", ("modest", "hostile"))
@pytest.mark.parametrize("name", ("cornell", "hand"))
def test_every_ray_passes_through_its_point_of_the_plane_of_focus(cases, settings, rvs, name, lens):
    """In float64, the ray (o, d) meets the plane dot(x - position, forward) = focal_dist at position + v focal_dist, within
    2e-6 (focal_dist |v| + |position|): a handful of float32 roundings of 6e-8 each, relative to the two lengths that enter; a plain
    float32 restatement measured 3.3e-7 at worst over 800,000 random rays, cameras and scales, and the bound is six times that."""
    mesh, _, cam = cases[name]
    scene = ir.RefScene(mesh, cam, W, H)
    a, fd = settings[(name, lens)]
    pos, fwd = scene.cam_pos.astype(np.float64), scene.cam_forward.astype(np.float64)
    worst = 0.0
    for rx, ry in rvs:
        r = lr.lens_rays(scene, rx, ry, a, fd)
        o, d, v = (r[k].astype(np.float64) for k in ("o", "d", "v"))
        t = (float(fd) - (o - pos) @ fwd) / (d @ fwd)
        hit = o + d * t[:, None]
        want = pos + v * float(fd)
        err = np.linalg.norm(hit - want, axis=1)
        bound = 2e-6 * (float(fd) * np.linalg.norm(v, axis=1) + np.linalg.norm(pos))
        worst = max(worst, float((err / bound).max()))
        assert (t > 0).all() and (err <= bound).all(), (name, lens, float(err.max()), float(bound.min()))
    print(name, lens, "worst error / bound:", worst)


@pytest.mark.parametrize("lens", ("modest", "hostile"))
def test_lens_points_lie_on_the_disc_in_every_quadrant(cases, settings, rvs, lens):
    mesh, _, cam = cases["hand"]
    scene = ir.RefScene(mesh, cam, W, H)
    a, fd = settings[("hand", lens)]
    for rx, ry in rvs:
        r = lr.lens_rays(scene, rx, ry, a, fd)
        lx, ly = r["lx"].astype(np.float64), r["ly"].astype(np.float64)
        assert (lx * lx + ly * ly <= float(a) ** 2 * (1 + 1e-6)).all()
        for sx in (1, -1):
            for sy in (1, -1):
                assert ((lx * sx > 0) & (ly * sy > 0)).sum() > W * H // 8          # a quarter each, give or take
        # the origin is position + right lx + up ly, and the RNG went on two draws behind the pinhole's
        assert np.array_equal(bits(r["o"]), bits(scene.cam_pos + (scene.cam_right * r["lx"][:, None] + scene.cam_up * r["ly"][:, None]).astype(f32)))
        pin = ir.primary_rays(scene, rx, ry)[2]
        everyone = np.ones(W * H, bool)
        pin.draw(everyone)
        pin.draw(everyone)
        assert np.array_equal(bits(pin.sx), bits(r["rng"].sx)) and np.array_equal(bits(pin.sy), bits(r["rng"].sy))


@pytest.mark.parametrize("lens", ("modest", "hostile"))
def test_a_lens_frame_differs_from_the_pinhole_frame(reference, lens):
    for depth in (1, 3):
        a, b = reference[("hand", lens)][0][depth - 1], reference[("hand", "pinhole")][0][depth - 1]
        differing = int((bits(a) != bits(b)).sum())
        print(lens, depth, "differing words:", differing, "of", a.size)
        assert differing >= a.size // 4, (lens, depth, differing)


# ---------------------------------------------------------------------------------------------- GPU: rays

def ray_rows(o, tmax, d):
    """28-byte rows (o, tmax, d), sorted: a multiset"""
    a = np.concatenate([bits(o).reshape(-1, 3), bits(tmax).reshape(-1, 1), bits(d).reshape(-1, 3)], 1)
    return sorted(r.tobytes() for r in a)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", (1, 3))
@pytest.mark.parametrize("lens", ("modest", "hostile"))
def test_gpu_primary_rays_equal_the_reference(cr, cases, settings, rvs, lens, depth):
    """k_raygen_lens' queue after one frame, as a multiset of (o, tmax, d) rows: lens_ref's rays bit for bit, tmax 1e9f.  At depth 3 too:
    no later segment of the frame writes over the primary rays."""
    mesh, data, cam = cases["hand"]
    a, fd = settings[("hand", lens)]
    scene = cr.Scene(data, W, H, depth)
    try:
        scene.update(lens_camera(cr, cam, a, fd))
        rx, ry = rvs[0]
        scene.render_frame(rx, ry)
        got = scene.debug_read_queue(0, 0)
        want = lr.lens_rays(ir.RefScene(mesh, cam, W, H), rx, ry, a, fd)
        assert got.shape[0] == W * H
        assert (bits(got["tmax"]) == bits(f32(1e9))).all()
        assert ray_rows(got["o"], got["tmax"], got["d"]) == ray_rows(want["o"], np.full(W * H, 1e9, f32), want["d"])
        n_tiles, tile, _ = scene.packed_info()                                 # the payload: the path's id, here its local pixel (tile-major)
        ids = got["pad"].tolist()
        assert len(set(ids)) == W * H and max(ids) < n_tiles * tile * tile
    finally:
        scene.close()


# ---------------------------------------------------------------------------------------------- GPU: frames

def render_and_check(cr, data, cam, lens_setting, entry, rvs, depth, options=(), one_call=False, devices=None, expect_samples=None):
    sums, per_frame, total = entry
    scene = cr.Scene(data, W, H, depth)
    try:
        if devices is not None:
            scene.set_devices(devices)
        for k, v in options:
            scene.set_option(k, v)
        scene.update(lens_camera(cr, cam, *lens_setting))
        if one_call:
            scene.render_frames(rvs)
            st = scene.frame_stats()
            info = scene.launch_info()
            assert info[0] == 0 and info[1] == 16 and info[2] == (len(rvs) if expect_samples is None else expect_samples), info
            if info[2] == len(rvs):                                    # one chain: the stats describe all of it
                assert (st["closest_rays"], st["any_rays"]) == (total[depth - 1]["closest_rays"], total[depth - 1]["shadow_rays"])
        else:
            for f, (rx, ry) in enumerate(rvs):
                scene.render_frame(rx, ry)
                st = scene.frame_stats()
                assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
            info = scene.launch_info()
            assert info[:3] == [0, 16, 1], info
        assert st["stack_overflows"] == 0
        got = scene.read_sum()
        differing = int((bits(got) != bits(sums[depth - 1])).sum())
        assert differing == 0, differing
        scene.frame_count = len(rvs)
        rgba = scene.resolve()
        assert np.array_equal(rgba, ir.resolve_ref(got, f32(1.0 / len(rvs))))
        assert np.array_equal(rgba, ir.resolve_ref(sums[depth - 1], f32(1.0 / len(rvs))))
    finally:
        scene.close()


GPU_CASES = [(n, "modest", d) for n in ("cornell", "tess8", "textured", "hand_unlit") for d in (1, 3)] + \
            [("hand", lens, d) for lens in ("modest", "hostile") for d in (1, 2, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,lens,depth", GPU_CASES)
def test_gpu_frames_equal_the_reference(cr, cases, settings, rvs, reference, name, lens, depth):
    """the sums after four render_frame calls as uint32 words, each frame's closest and shadow ray counts against the census, and the
    resolved bytes against resolve_ref.  tess8 is the tree of more than 64 node8s: the voting loop and the deferred shadow walk."""
    _, data, cam = cases[name]
    render_and_check(cr, data, cam, settings[(name, lens)], reference[(name, lens)], rvs, depth)


VARIANTS = ("render_frames", "render_frames_depth_1", "inplace_shadow_0", "inplace_shadow_1", "inplace_shadow_2", "bounce_refill_1", "bvh2_frame_mode",
            "device_built_sah", "two_devices", "streams_2", "jitter_0", "count_visits_1")


@pytest.mark.gpu
@pytest.mark.parametrize("variant", VARIANTS)
def test_gpu_variants_equal_the_reference(cr, cases, settings, rvs, reference, variant):
    """Scene (d) through the modest lens, paths of 3 segments, once through each other way to the same frame"""
    name, depth, kw, ref_lens = "hand", 3, {}, "modest"
    data = cases[name][1]
    if variant == "render_frames":
        kw = {"one_call": True}
    elif variant == "render_frames_depth_1":
        depth, kw = 1, {"one_call": True}
    elif variant.startswith("inplace_shadow_"):
        kw = {"options": (("inplace_shadow", int(variant[-1])),)}
    elif variant == "bounce_refill_1":
        kw = {"options": (("bounce_refill", 1),)}
    elif variant == "bvh2_frame_mode":
        name, kw = "hand_lambert", {"options": (("accel", 1),)}          # the BVH2 frame mode is the Lambert-only shader
        data = cases[name][1]
    elif variant == "device_built_sah":
        data = cr.SceneData.for_device_build(cases["hand"][0], cases["hand"][2], "sah")
    elif variant == "two_devices":
        kw = {"devices": [0, 0]}
    elif variant == "streams_2":
        kw = {"options": (("streams", 2),)}
    elif variant == "jitter_0":
        ref_lens, kw = "modest_nojitter", {"options": (("jitter", 0),)}
    else:
        kw = {"options": (("count_visits", 1),)}
    render_and_check(cr, data, cases[name][2], settings[(name, "modest")], reference[(name, ref_lens)], rvs, depth, **kw)


@pytest.mark.gpu
def test_gpu_tile_shards_add_up_to_the_frame(cr, cases, settings, rvs, reference):
    """crt_set_shard: the two halves of the tiles, rendered by two scenes, hold the reference's words where they have pixels and zero elsewhere"""
    _, data, cam = cases["hand"]
    want = reference[("hand", "modest")][0][2]
    got = np.zeros((H, W, 3), f32)
    covered = np.zeros((H, W), np.int64)
    for rank in (0, 1):
        scene = cr.Scene(data, W, H, 3)
        try:
            scene.set_shard(rank, 2, 8)
            scene.update(lens_camera(cr, cam, *settings[("hand", "modest")]))
            for rx, ry in rvs:
                scene.render_frame(rx, ry)
            part = scene.read_sum()
            got += part
            covered += (part != 0).any(-1)
        finally:
            scene.close()
    assert covered.max() == 1 and np.array_equal(bits(got), bits(want + f32(0.0)))


# ---------------------------------------------------------------------------------------------- GPU: back to the pinhole

@pytest.mark.gpu
def test_gpu_aperture_back_to_zero_is_the_pinhole(cr, cases, settings, rvs, reference):
    _, data, _ = cases["hand"]
    cam = hand_made_mesh(cr)[1]                                          # a Camera of its own: set_lens changes it
    sums = reference[("hand", "pinhole")][0]
    scene = cr.Scene(data, W, H, 3)
    try:
        scene.update(cam.set_lens(*settings[("hand", "modest")]))
        for rx, ry in rvs[:2]:
            scene.render_frame(rx, ry)
        assert scene.launch_info()[1] == 16
        scene.reset()
        scene.update(cam.set_lens(0.0, 1.5))
        for rx, ry in rvs:
            scene.render_frame(rx, ry)
        assert scene.launch_info()[1] & 16 == 0
        assert int((bits(scene.read_sum()) != bits(sums[2])).sum()) == 0
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_launch_form_after_a_lens_is_a_fresh_scenes(cr, cases, settings, rvs, reference):
    """tess8, one segment, four frames in one call: after lens frames and set_lens(0, ...) the launch is the one a fresh scene makes, and
    the bytes are the pinhole reference's"""
    _, data, cam = cases["tess8"]
    fresh = cr.Scene(data, W, H, 1)
    scene = cr.Scene(data, W, H, 1)
    try:
        fresh.render_frames(rvs)
        want_info = fresh.launch_info()
        scene.update(lens_camera(cr, cam, *settings[("tess8", "modest")]))
        scene.render_frames(rvs)
        assert scene.launch_info()[:3] == [0, 16, 4]
        scene.reset()
        scene.update(lens_camera(cr, cam, 0.0, float(settings[("tess8", "modest")][1])))
        scene.render_frames(rvs)
        assert scene.launch_info() == want_info and want_info[1] & 16 == 0
        got = scene.read_sum()
        assert np.array_equal(bits(got), bits(fresh.read_sum()))
        assert int((bits(got) != bits(reference[("tess8", "pinhole")][0][0])).sum()) == 0
    finally:
        fresh.close()
        scene.close()


# ---------------------------------------------------------------------------------------------- GPU: AOVs

@pytest.mark.gpu
def test_gpu_aovs_do_not_depend_on_the_aperture(cr, cases, rvs):
    from caitlynrenderer_amd.scene import AOV_ALL
    _, data, cam = cases["hand"]
    scene = cr.Scene(data, W, H, 3)
    try:
        out = []
        for a, fd in ((0.0, 0.5), HOSTILE):
            scene.update(lens_camera(cr, cam, a, fd))
            scene.render_frame(*rvs[0])                                  # a frame in between changes nothing either
            scene.render_aov(rvs[1][0], rvs[1][1], AOV_ALL)
            out.append([np.ascontiguousarray(scene.read_aov(1 << k)).tobytes() for k in range(5)])
        for k in range(5):
            assert out[0][k] == out[1][k], k
    finally:
        scene.close()


# ---------------------------------------------------------------------------------------------- GPU: instanced scenes

def lens_yard(cr):
    """Two meshes, three instances: a box as the ground (material offset 1), the box again rotated and non-uniformly scaled, and a lamp mesh
    — a quad of two triangles, one light each — turned a little: a mesh light that follows its instance."""
    mats = np.array([material((0.8, 0.5, 0.3)), material((0.6, 0.6, 0.6)), material(emission=(9.0, 8.0, 7.0), ew=0.0),
                     material(emission=(9.0, 8.0, 7.0), ew=1.0)], f32)
    meshes = [box_mesh(cr, 0, mats),
              quad_mesh(cr, (-1.5, 0.0, -1.1), (0, 0, 2.2), (3.0, 0, 0), (2, 3), normal=(0, -1, 0), mats=mats, fourth=0.6)]
    lamp_lights = quad_lights(meshes[1], (0, -1, 0), (9.0, 8.0, 7.0))
    inst = [(place(np.diag([12.0, 0.5, 12.0]), (0.0, -0.5, 1.0)), 0, 0xfe, 1),                              # hidden from primary rays when masks are on
            (place(rot((0, 1, 0), 0.5) @ np.diag([1.4, 1.7, 1.0]), (0.6, 0.0, 0.9)), 0, 0xff, 0),
            (place(rot((0, 0, 1), 0.2) @ rot((0, 1, 0), 0.4), (0.2, 2.6, 0.8)), 1, 0xfb, 0)]                # hidden from shadow rays
    cam = cr.Camera((0.4, 3.6, -8.4), (0.0, 1.1, 1.2), 50.0)
    return types.SimpleNamespace(meshes=meshes, M=np.array([i[0] for i in inst], f32), mesh_of=np.array([i[1] for i in inst]),
                                 masks=np.array([i[2] for i in inst], np.uint32), offsets=np.array([i[3] for i in inst], np.uint32),
                                 mats=mats, static=np.zeros((0, 18), f32), mesh_lights=[None, lamp_lights], textures=None, cam=cam)


INST_LENS = (f32(0.12), f32(9.0))       # focused near the boxes, the ground in front and behind out of focus
INST_MASKS = {"instance_masks": 1, "mask_primary": 0x01, "mask_bounce": 0x02, "mask_shadow": 0x04}


@pytest.fixture(scope="module")
def inst_reference(cr, rvs):
    import instanced_ref as xr
    s = lens_yard(cr)

    def make(masks):
        ref = xr.InstancedRef(s.meshes, s.M, s.mesh_of, s.masks, s.offsets, s.mats, s.static, s.mesh_lights, s.textures, s.cam, W, H,
                              options=INST_MASKS if masks else None)
        sums, _, total, per_frame = lr.render(ref, rvs, 3, *INST_LENS)
        return _frozen(sums), per_frame, total
    return s, _Lazy(make)


def test_instanced_lens_reference_sees_the_scene(inst_reference):
    """conditions on the scene, in the reference alone: it is lit, its paths bounce, shadow rays are cast and some are blocked, and the
    masks change what primary rays see"""
    _, ref = inst_reference
    c = ref[False][2][2]
    assert ref[False][0][2].max() > 0.4 and c["shadow_occluded"] >= 20 and c["shadow_clear"] >= 20 and c["hits_general_primary"] >= 20
    assert c["hits_with_offset"] >= 20 and c["nee_moved_light"] >= 20
    assert ref[True][2][2]["mask_changes_primary"] >= 20


@pytest.mark.gpu
@pytest.mark.parametrize("masks", (False, True))
@pytest.mark.parametrize("depth", (1, 3))
def test_gpu_instanced_frames_equal_the_reference(cr, inst_reference, rvs, depth, masks):
    s, ref = inst_reference
    sums, per_frame, _ = ref[masks]
    inst = cr.InstancedScene(s.meshes, cr.instances_array(s.M, s.mesh_of, masks=s.masks, material_offsets=s.offsets), builder="sah")
    sc = inst.frame_scene(shading_of(s.meshes), s.mats, s.static, W, H, depth, textures=None, mesh_lights=s.mesh_lights)
    try:
        for k, v in (INST_MASKS if masks else {}).items():
            sc.set_option(k, v)
        sc.update(lens_camera(cr, s.cam, *INST_LENS))
        for f, (rx, ry) in enumerate(rvs):
            sc.render_frame(rx, ry)
            st = sc.frame_stats()
            assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
        assert sc.launch_info()[:3] == [0, 16, 1]
        assert int((bits(sc.read_sum()) != bits(sums[depth - 1])).sum()) == 0
    finally:
        sc.close()
        inst.close()


# ---------------------------------------------------------------------------------------------- GPU: crt_set_camera's refusals

REFUSED = (("aperture", float("nan"), 1.5), ("aperture", float("inf"), 1.5), ("aperture", -0.01, 1.5),
           ("focal_dist", 0.03, 0.0), ("focal_dist", 0.03, -1.0), ("focal_dist", 0.03, float("nan")), ("focal_dist", 0.03, float("inf")))


@pytest.mark.gpu
@pytest.mark.parametrize("devices", (None, [0, 0]))
def test_gpu_set_camera_refuses_a_bad_lens_and_keeps_the_camera(cr, cases, settings, rvs, reference, devices):
    from caitlynrenderer_amd._lib import CrtError
    _, data, cam = cases["hand"]
    want = reference[("hand", "modest")][0][0]
    one = lr.render(ir.RefScene(cases["hand"][0], cam, W, H), rvs[:1], 1, *settings[("hand", "modest")])[0][0]
    scene = cr.Scene(data, W, H, 1)
    try:
        if devices is not None:
            scene.set_devices(devices)
        scene.update(lens_camera(cr, cam, *settings[("hand", "modest")]))
        for field, a, fd in REFUSED:
            with pytest.raises(CrtError) as e:
                scene.update(lens_camera(cr, cam, a, fd))
            assert field in str(e.value), (field, str(e.value))
            scene.reset()
            scene.render_frame(*rvs[0])
            assert int((bits(scene.read_sum()) != bits(one)).sum()) == 0, (field, a, fd)     # the previous camera's bytes
        scene.update(lens_camera(cr, cam, 0.0, float("nan")))                               # a pinhole: focal_dist is not looked at
        scene.update(lens_camera(cr, cam, 0.0, -3.0))
        scene.update(lens_camera(cr, cam, *settings[("hand", "modest")]))
        scene.reset()
        for rx, ry in rvs:
            scene.render_frame(rx, ry)
        assert int((bits(scene.read_sum()) != bits(want)).sum()) == 0
    finally:
        scene.close()
