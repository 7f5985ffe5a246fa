"""crt_display (include/crt.h) against tests/display_ref.py: the bins, the state (counted, q, the bits of metered and exposure)
and the RGBA8 bytes, always on the image read back from the device.  The CPU half checks display_ref against integrator_ref's resolve, the
meter's arithmetic on hand-made counts and the census of the frames the GPU half meters: at least 8 occupied bins and at least one pixel that
does not count."""
import ctypes as C
import math

import numpy as np
import pytest

import display_ref as dr
import env_ref as er
import integrator_ref as ir

f32 = np.float32
W, H = 44, 28                    # 1232 pixels: no multiple of 256 or 64, so the tails run
FRAMES = 4
INV = f32(1.0 / FRAMES)
ADAPT_INVS = (1.0, 0.25, 4.0, 1.0, 1.0)


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def bits_of(x):
    return int(np.array([x], f32).view(np.uint32)[0])


# ---------------------------------------------------------------------------------------------- the frames, computed once

def edge_values():
    """grey values for every bin edge (the float below, the edge, the float above) and the values the meter must leave out or clamp"""
    edges = ((dr.FIRST_BIN + np.arange(256, dtype=np.int64)) << 20)
    around = (edges[:, None] + np.array([-1, 0, 1])[None, :]).reshape(-1).astype(np.uint32).view(f32)
    special = np.array([0.0, -1.0, 1e-41, 2.0 ** -16, np.nextafter(f32(2.0 ** -16), f32(0)), 65535.0, 1e6, np.inf, np.nan], f32)
    return np.concatenate([around, special]).astype(f32)


def edge_pixels():
    v = edge_values()
    return np.stack([v, v, v], -1)


WALL_COLS = 28


def wall_image():
    """the sum a one-segment frame of emitter_wall(edge_pixels()) holds, as the reference knows it without a device: quad q's value in its
    3 x 3 pixels, 0.25 in the quads beyond the set"""
    px = edge_pixels()
    rows = -(-px.shape[0] // WALL_COLS)
    quads = np.full((rows * WALL_COLS, 3), 0.25, f32)
    quads[:px.shape[0]] = px
    return np.repeat(np.repeat(quads.reshape(rows, WALL_COLS, 3), 3, 0), 3, 1)


def hdr_env():
    """a 16 x 16 map with one texel at 5000 and the rest below 1, hidden from the camera: the backdrop stays 0 and does not count"""
    rng = np.random.default_rng(29)
    t = (0.05 + 0.9 * rng.random((16, 16, 3))).astype(f32)
    t[5, 9] = 5000.0
    return er.Env(t, None, (1.0, 1.0, 1.0), hide_from_camera=True)


def set_env(scene, env):
    scene.set_environment(env.texels, env.rotation, tuple(float(x) for x in env.scale), env.hide_from_camera)


@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def hdr(cr):
    """§28's cube on its ground quad: (mesh, SceneData, camera, environment)"""
    from test_environment import cube_quad_scene
    mesh, cam = cube_quad_scene(cr)
    return mesh, cr.SceneData.build(mesh, cam), cam, hdr_env()


@pytest.fixture(scope="module")
def hdr_reference(hdr, rvs):
    """the sum of four frames at depth 3 from the numpy integrator alone"""
    mesh, _, cam, env = hdr
    s = er.render(ir.RefScene(mesh, cam, W, H), rvs, 3, env)[0][2]
    s.setflags(write=False)
    return s


def hdr_scene(cr, hdr, rvs, depth=3, before=None, width=W, height=H):
    _, data, cam, env = hdr
    scene = cr.Scene(data, width, height, depth)
    try:
        if before is not None:
            before(scene)
        scene.update(cam)
        set_env(scene, env)
        scene.render_frames(rvs)
    except Exception:
        scene.close()
        raise
    return scene


def check_call(scene, image, inv, p, meter, owned=None):
    """one display() against the reference on `image`: bytes, state and, when it meters, the bins.  Returns (rgba, state)."""
    want, state, hist = dr.display(image, inv, p, meter, owned)
    got = scene.display(inv, **p.kwargs())
    st = scene.display_state()
    assert (st["counted"], st["q"], st["calls"]) == (state["counted"], state["q"], state["calls"]), (st, state)
    assert bits_of(st["metered"]) == bits_of(state["metered"]) and bits_of(st["exposure"]) == bits_of(state["exposure"]), (st, state)
    if p.auto:
        assert scene.display_histogram().tolist() == hist
    bad = np.nonzero((got != want).any(-1))
    assert bad[0].size == 0, (p.curve, p.auto, state["exposure"], bad[0].size, np.asarray(image)[bad][:3], got[bad][:3], want[bad][:3])
    return got, state


# ---------------------------------------------------------------------------------------------- CPU: the reference itself

@pytest.mark.parametrize("inv", (1.0, 1.0 / 3.0))
def test_reference_curve_at_exposure_one_is_resolve_ref(inv):
    from test_integrator_ref import resolve_set
    px = resolve_set(f32(inv))
    got, state, hist = dr.display(px, f32(inv), dr.Params(), dr.Meter())
    assert np.array_equal(got, ir.resolve_ref(px, f32(inv)))
    assert hist is None and state["exposure"] == f32(1.0) and state["calls"] == 0


def test_a_flat_image_meters_to_its_luminance():
    p = dr.Params(auto=True)
    for e in range(-16, 16):
        for m in (1.0, 1.03, 1.37, 1.9999):
            L = f32(m * 2.0 ** e)
            st = dr.meter_call(dr.histogram(np.full(100, L, f32)), p, dr.Meter())
            assert st["counted"] == 100 and 0.94 * float(L) < float(st["metered"]) <= 1.0625 * float(L), (L, st)
    # four figures checked by hand
    for L, want in ((0.01, 0.01025), (0.18, 0.17969), (3.7, 3.625), (1000.0, 992.0)):
        st = dr.meter_call(dr.histogram(np.full(7, L, f32)), p, dr.Meter())
        assert abs(float(st["metered"]) - want) <= 6e-4 * want, (L, st)


def test_bins_at_the_ends():
    L = np.array([2.0 ** 16, 1e6, 3e38, 65535.0, 2.0 ** -16, np.nextafter(f32(2.0 ** -16), f32(0)), 0.0, -1.0, np.inf, -np.inf, np.nan, 1e-41], f32)
    assert dr.bins_of(L).tolist() == [255, 255, 255, 255, 0, -1, -1, -1, -1, -1, -1, -1]
    assert dr.bins_of(np.array([1.0, 1.125, 1.99, 2.0], f32)).tolist() == [128, 129, 135, 136]


def test_trims_on_hand_made_counts():
    h = [0] * 256
    h[10], h[20], h[200] = 500, 400, 100
    assert dr.trimmed(h, 0, 1000) == (1000, 1000, 500 * 10 + 400 * 20 + 100 * 200)
    assert dr.trimmed(h, 500, 950) == (1000, 450, 400 * 20 + 50 * 200)
    assert dr.trimmed(h, 0, 1) == (1000, 1, 10)
    few = [0] * 256
    few[7] = 999
    assert dr.trimmed(few, 0, 1) == (999, 0, 0)
    p, meter = dr.Params(auto=True, exposure=3.0, low_permille=0, high_permille=1), dr.Meter()
    st = dr.meter_call(few, p, meter)                      # M == 0 and no exposure yet: params.exposure, calls stays 0
    assert (st["exposure"], st["metered"], st["counted"], st["q"], st["calls"]) == (f32(3.0), f32(0.0), 999, 0, 0)
    first = dr.meter_call(h, dr.Params(auto=True), meter)
    assert first["calls"] == 1 and first["q"] == (500 * 10 + 400 * 20 + 100 * 200) * 256 // 1000 + 128
    st = dr.meter_call(few, p, meter)                      # M == 0 afterwards: the exposure carries over
    assert st["exposure"] == first["exposure"] and st["calls"] == 1 and st["metered"] == f32(0.0)


def test_adaptation_recurrence_and_clamps():
    meter, E = dr.Meter(), []
    for k, L in enumerate((0.18, 1.0, 1.0, 0.01, 0.01)):
        st = dr.meter_call(dr.histogram(np.full(10, L, f32)), dr.Params(auto=True, adapt=0.25), meter)
        target = f32(f32(0.18) / st["metered"])
        want = target if k == 0 else f32(E[-1] + f32(f32(target - E[-1]) * f32(0.25)))
        assert bits_of(st["exposure"]) == bits_of(want) and st["calls"] == k + 1
        E.append(st["exposure"])
    assert E[1] < E[0] and E[2] < E[1] and E[3] > E[2]
    st = dr.meter_call(dr.histogram(np.full(10, 1.0, f32)), dr.Params(auto=True, adapt=1.0), meter)
    assert bits_of(st["exposure"]) == bits_of(f32(f32(0.18) / st["metered"]))               # adapt == 1: exactly E_target
    lo = dr.meter_call(dr.histogram(np.full(10, 1000.0, f32)), dr.Params(auto=True, exposure_min=0.5, exposure_max=2.0), dr.Meter())
    hi = dr.meter_call(dr.histogram(np.full(10, 0.001, f32)), dr.Params(auto=True, exposure_min=0.5, exposure_max=2.0), dr.Meter())
    assert lo["exposure"] == f32(0.5) and hi["exposure"] == f32(2.0)


def test_curves_rise_and_aces_by_hand():
    # As float32 values the curves rise wherever a step's rise exceeds the rounding of the last division (an ulp of 1: 1.2e-7).  The flattest
    # is ACES near its ceiling, y ~ 1.033 - 0.2 / x: on 0 .. 8 in steps of 1 / 32 at E = 37.5, x reaches 300 and a step still rises by
    # 0.2 * 1.17 / 300^2 = 2.6e-6.  On a ramp 64 times denser and 8 times longer it is the BYTES that must not fall.
    ramp = np.linspace(0.0, 8.0, 257).astype(f32)
    dense = np.linspace(0.0, 64.0, 4097).astype(f32)
    for name in dr.CURVES:
        for E in (0.25, 1.0, 37.5):
            y = dr.curve(np.stack([ramp, ramp, ramp], -1), f32(E), dr.Params(curve=name, white=4.0))[:, 0]
            assert (np.diff(y) >= 0).all(), (name, E)
            b = dr.gamma_bytes(dr.curve(np.stack([dense, dense, dense], -1), f32(E), dr.Params(curve=name, white=4.0))[:, 0])
            assert (np.diff(b.astype(np.int64)) >= 0).all(), (name, E)
    # Narkowicz's fit at three points, in exact rationals: x (2.51 x + 0.03) / (x (2.43 x + 0.59) + 0.14)
    y = dr.curve(np.array([[0.0, 1.0, 0.5]], f32), f32(1.0), dr.Params(curve="aces"))[0]
    assert y[0] == 0.0
    assert abs(float(y[1]) - 2.54 / 3.16) < 1e-6 and abs(float(y[2]) - 0.6425 / 1.0425) < 1e-6
    one = dr.curve(np.array([[4.0, 4.0, 4.0]], f32), f32(1.0), dr.Params(curve="reinhard", white=4.0))[0]
    assert abs(float(one[0]) - 1.0) < 1e-6                                               # Reinhard maps the white point to 1
    assert dr.gamma_bytes(np.array([-np.inf, -1.0, np.nan, 0.0, 1.0, np.inf], f32)).tolist() == [0, 0, 0, 0, 255, 255]


def test_census_of_the_metered_frames(hdr_reference):
    """from the reference alone: each metered frame has at least 8 occupied bins and at least one pixel that does not count"""
    occupied, left_out = dr.census(wall_image(), f32(1.0))
    assert occupied == 256 and left_out >= 9 * 5, (occupied, left_out)
    for inv in sorted(set(ADAPT_INVS)):
        occupied, left_out = dr.census(hdr_reference, f32(inv) * INV)
        assert occupied >= 8 and left_out >= 1, (inv, occupied, left_out)
    # fewer than 1000 pixels count, so the trim (0, 1) keeps none of them
    counts = dr.histogram(dr.luminance(dr.input_pixels(hdr_reference, INV)))
    assert 0 < sum(counts) < 1000 and dr.trimmed(counts, 0, 1)[1] == 0 and dr.trimmed(counts, 500, 950)[1] > 0
    # under ACES with a metered exposure fewer bytes saturate than under the fixed curve
    aces = dr.display(hdr_reference, INV, dr.Params(curve="aces", auto=True), dr.Meter())[0]
    fixed = ir.resolve_ref(hdr_reference, INV)
    assert int((aces[..., :3] == 255).sum()) < int((fixed[..., :3] == 255).sum())


# ---------------------------------------------------------------------------------------------- GPU

@pytest.mark.gpu
def test_gpu_every_bin_edge(cr):
    from test_integrator_ref import emitter_wall
    px = edge_pixels()
    rows = -(-px.shape[0] // WALL_COLS)
    mesh, cam, width, height = emitter_wall(cr, px, WALL_COLS, rows)
    scene = cr.Scene(cr.SceneData.build(mesh, cam), width, height, 1)
    try:
        scene.render_frame(0.37, 0.61)
        got = scene.read_sum()
        finite = np.isfinite(px).all(1) & (px != 0).all(1) & (np.abs(px) > 1e-30).all(1)
        seen = {r.tobytes() for r in bits(got).reshape(-1, 3)}
        assert all(r.tobytes() in seen for r in bits(px[finite])), "every finite value of the set reaches the sum"
        occupied, left_out = dr.census(got, f32(1.0))
        assert occupied == 256 and left_out >= 1
        for curve in dr.CURVES:
            _, st = check_call(scene, got, f32(1.0), dr.Params(curve=curve, auto=True), dr.Meter())
            scene.display_reset()
            assert st["counted"] == got.shape[0] * got.shape[1] - left_out
            for E in (0.25, 1.0, 37.5):
                check_call(scene, got, f32(1.0), dr.Params(curve=curve, exposure=E), dr.Meter())
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ("cornell", "tess8", "textured"))
def test_gpu_reference_curve_is_the_resolve_kernel(cr, cornell, cornell_data, tess8, textured, rvs, name):
    from test_denoise import device_bytes_at
    data, cam = {"cornell": (cornell_data, cornell[1]), "tess8": (tess8[1], cornell[1]), "textured": (textured[1], textured[2])}[name]
    scene = cr.Scene(data, W, H, 3)
    try:
        scene.update(cam)
        scene.render_frames(rvs)
        want = scene.resolve(INV)
        p = scene.resolve_device(INV)
        assert np.array_equal(scene.display(INV, curve="reference", exposure=1.0), want)
        from caitlynrenderer_amd import _lib
        _lib.check(_lib.lib().crt_display(scene._h, float(INV), None, 1))                 # NULL params: the header's defaults
        assert np.array_equal(scene.read_display(), want)
        assert np.array_equal(scene.display(INV), want)                                    # and the binding's
        assert scene.display_device() != p
        assert np.array_equal(device_bytes_at(p, W * H * 4), want.reshape(-1))              # resolve_device's bytes are what they were
        assert np.array_equal(want, ir.resolve_ref(scene.read_sum(), INV))
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_hdr_environment(cr, hdr, rvs):
    scene = hdr_scene(cr, hdr, rvs)
    try:
        got = scene.read_sum()
        occupied, left_out = dr.census(got, INV)
        assert occupied >= 8 and left_out >= 1
        out = {}
        for curve in dr.CURVES:
            out[curve], _ = check_call(scene, got, INV, dr.Params(curve=curve, auto=True, white=2.0), dr.Meter())
            scene.display_reset()
        assert int((out["aces"][..., :3] == 255).sum()) < int((scene.resolve(INV)[..., :3] == 255).sum())
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_adaptation(cr, hdr, rvs):
    scene = hdr_scene(cr, hdr, rvs)
    try:
        got = scene.read_sum()
        meter = dr.Meter()
        p = dr.Params(curve="aces", auto=True, adapt=0.25)
        seen = []
        for k, inv in enumerate(ADAPT_INVS):
            _, st = check_call(scene, got, f32(inv) * INV, p, meter)
            seen.append(st["exposure"])
            if k == 2:                                     # a manual call in between leaves the adaptation as it was
                _, manual = check_call(scene, got, INV, dr.Params(curve="aces", exposure=2.5), meter)
                assert manual["exposure"] == f32(2.5) and manual["calls"] == 3
        assert len({bits_of(e) for e in seen}) == len(seen) and meter.calls == 5
        scene.display_reset()
        meter.reset()
        _, st = check_call(scene, got, INV, p, meter)    # the first-call rule again: E_target itself
        assert st["calls"] == 1 and bits_of(st["exposure"]) == bits_of(f32(f32(0.18) / st["metered"]))
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_trims_and_the_empty_meter(cr, hdr, rvs):
    scene = hdr_scene(cr, hdr, rvs)
    try:
        got = scene.read_sum()
        meter = dr.Meter()
        _, empty = check_call(scene, got, INV, dr.Params(auto=True, exposure=3.0, low_permille=0, high_permille=1), meter)
        assert empty["calls"] == 0 and empty["counted"] > 0 and empty["exposure"] == f32(3.0)         # fewer than 1000 counted: M == 0
        _, full = check_call(scene, got, INV, dr.Params(auto=True), meter)
        _, cut = check_call(scene, got, INV, dr.Params(auto=True, low_permille=500, high_permille=950), meter)
        assert cut["q"] != full["q"] and cut["calls"] == 2
        _, kept = check_call(scene, got, INV, dr.Params(auto=True, exposure=3.0, low_permille=0, high_permille=1), meter)
        assert kept["calls"] == 2 and bits_of(kept["exposure"]) == bits_of(cut["exposure"])             # M == 0: E carries over
    finally:
        scene.close()
    # a scene that hits nothing, without an environment: N == 0
    _, data, cam, _ = hdr
    away = cr.Camera((0.0, 5.0, -10.0), (0.0, 50.0, -10.5), 20.0)
    scene = cr.Scene(data, W, H, 3)
    try:
        scene.update(away)
        scene.render_frames(rvs)
        got = scene.read_sum()
        assert not got.any()
        rgba, st = check_call(scene, got, INV, dr.Params(auto=True, exposure=2.0), dr.Meter())
        assert (st["counted"], st["calls"], st["exposure"]) == (0, 0, f32(2.0))
        assert (rgba.reshape(-1, 4) == (0, 0, 0, 255)).all()
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_sources(cr, hdr, rvs):
    from caitlynrenderer_amd.scene import AOV_ALL
    scene = hdr_scene(cr, hdr, rvs)
    try:
        scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
        scene.denoise(INV, passes=3)
        scene.temporal(INV, source="sum")
        from test_denoise import device_bytes_at
        for source, read, resolve, resolve_device in (("denoised", scene.read_denoised, scene.resolve_denoised, scene.resolve_denoised_device),
                                                      ("temporal", scene.read_temporal, scene.resolve_temporal, scene.resolve_temporal_device)):
            image, rgba = read(), resolve()
            d_rgba = resolve_device()                          # the stage's own RGBA8: read where it lies afterwards, not resolved again
            occupied, left_out = dr.census(image, INV, source)
            assert occupied >= 8 and left_out >= 1, (source, occupied, left_out)
            a, _ = check_call(scene, image, INV, dr.Params(source=source, curve="aces", auto=True), dr.Meter())
            scene.display_reset()
            b, _ = check_call(scene, image, f32(7.0), dr.Params(source=source, curve="aces", auto=True), dr.Meter())
            scene.display_reset()
            assert np.array_equal(a, b)                                # inv_count is ignored
            check_call(scene, image, INV, dr.Params(source=source, curve="reinhard", exposure=0.5), dr.Meter())
            assert np.array_equal(bits(read()), bits(image))
            assert d_rgba != scene.display_device() and np.array_equal(device_bytes_at(d_rgba, W * H * 4), rgba.reshape(-1))
    finally:
        scene.close()


def owned_pixels(rank, world, tile):
    from caitlynrenderer_amd import tiles
    own = np.zeros((H, W), bool)
    for tx, ty in tiles.shard_tiles_of_library(W, H, tile, rank, world):
        own[ty * tile:(ty + 1) * tile, tx * tile:(tx + 1) * tile] = True
    return own


FORMS = ("two_devices", "two_devices_late", "shard_0", "shard_1", "streams_2", "instanced", "1x1", "257x3")


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_gpu_forms_of_the_sum(cr, hdr, rvs, form):
    inst, owned, late, size = None, None, None, (W, H)
    if form == "instanced":
        from test_instances_frames import shading_of
        from test_lens import lens_yard
        s = lens_yard(cr)
        inst = cr.InstancedScene(s.meshes, cr.instances_array(s.M, s.mesh_of, masks=s.masks, material_offsets=s.offsets), builder="sah")
        scene = inst.frame_scene(shading_of(s.meshes), s.mats, s.static, W, H, 3, textures=None, mesh_lights=s.mesh_lights)
        scene.update(s.cam)
        set_env(scene, hdr[3])
        scene.render_frames(rvs)
    else:
        before = None
        if form == "two_devices":
            before = lambda sc: sc.set_devices([0, 0])
        elif form == "two_devices_late":
            late = [0, 0]
        elif form.startswith("shard_"):
            rank = int(form[-1])
            before = lambda sc: sc.set_shard(rank, 2, 8)
            owned = owned_pixels(rank, 2, 8)
        elif form == "streams_2":
            before = lambda sc: sc.set_option("streams", 2)
        elif form == "1x1":
            size = (1, 1)
        elif form == "257x3":
            size = (257, 3)
        scene = hdr_scene(cr, hdr, rvs, before=before, width=size[0], height=size[1])
    try:
        got = scene.read_sum()
        if size == (W, H):
            occupied, left_out = dr.census(got, INV)
            assert occupied >= 8 and left_out >= 1, (form, occupied, left_out)
        meter = dr.Meter()
        for curve in ("aces", "reference"):
            rgba, st = check_call(scene, got, INV, dr.Params(curve=curve, auto=True, adapt=0.5), meter, owned)
            if late is not None:                           # the devices set after the first display: the buffers and the adaptation stay
                scene.set_devices(late)
                scene.reset()
                scene.render_frames(rvs)
                assert np.array_equal(bits(scene.read_sum()), bits(got))
        if owned is not None:
            assert (rgba[~owned] == 0).all() and (rgba[owned][:, 3] == 255).all()
            assert st["counted"] <= int(owned.sum())
    finally:
        scene.close()
        if inst is not None:
            inst.close()


@pytest.mark.gpu
def test_gpu_ordering(cr, hdr, rvs):
    _, data, cam, env = hdr
    out = []
    for sync in (True, False):
        scene = cr.Scene(data, W, H, 3)
        try:
            scene.update(cam)
            set_env(scene, env)
            scene.render_frames(rvs, sync=sync)
            first = scene.display(INV, curve="aces", auto=True, sync=sync)
            assert (first is None) == (not sync)
            scene.sync()
            out.append((scene.read_display(), scene.display_state(), scene.display_histogram()))
        finally:
            scene.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])
    assert {k: bits_of(v) for k, v in out[0][1].items()} == {k: bits_of(v) for k, v in out[1][1].items()}


@pytest.mark.gpu
def test_gpu_display_leaves_everything_alone(cr, hdr, rvs):
    from caitlynrenderer_amd.scene import AOV_ALL
    from test_denoise import device_bytes_in_use
    scene = hdr_scene(cr, hdr, rvs)
    try:
        scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
        scene.render_frame(*rvs[0])
        scene.frame_count = FRAMES + 1

        def everything():
            st = scene.frame_stats()
            return (scene.read_packed().tobytes(), [np.ascontiguousarray(scene.read_aov(1 << k)).tobytes() for k in range(5)],
                    st, scene.launch_info(), scene.frame_count)

        before = everything()
        scene.display(INV, curve="aces", auto=True)
        p = scene.display_device()
        in_use = device_bytes_in_use()
        scene.display(INV, curve="reinhard", auto=True, adapt=0.5)
        scene.display(INV, curve="clamp", exposure=2.0)
        assert device_bytes_in_use() == in_use and scene.display_device() == p           # a later call allocates nothing
        assert everything() == before
        scene.render_frame(*rvs[0])
        assert scene.launch_info() == before[3]
    finally:
        scene.close()


def raw_params(**kw):
    from caitlynrenderer_amd._lib import crt_display_params
    p = crt_display_params()
    p.source, p.curve, p.flags, p.exposure, p.white, p.key, p.adapt = 0, 0, 0, 1.0, 4.0, 0.18, 1.0
    p.exposure_min, p.exposure_max, p.low_permille, p.high_permille, p.reserved = 1e-6, 1e6, 0, 1000, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def refusals():
    nan, inf = float("nan"), float("inf")
    out = [("source", dict(source=3)), ("curve", dict(curve=4)), ("flag", dict(flags=2)), ("flag", dict(flags=0x80000001)), ("reserved", dict(reserved=1))]
    out += [("exposure", dict(exposure=v)) for v in (nan, inf, 0.0, -1.0, 1e-10, 1e10)]
    out += [("white", dict(curve=c, white=v)) for c in (0, 1) for v in (nan, inf, 1e-4, 1e7)]
    out += [("key", dict(flags=1, key=v)) for v in (nan, inf, 1e-7, 1e7)]
    out += [("adapt", dict(flags=1, adapt=v)) for v in (nan, inf, 0.0, -0.5, 1.5)]
    out += [("exposure_min", dict(flags=1, exposure_min=v)) for v in (nan, inf, 1e-10)]
    out += [("exposure_max", dict(flags=1, exposure_max=v)) for v in (nan, inf, 1e10)]
    out += [("exposure_min", dict(flags=1, exposure_min=2.0, exposure_max=1.0))]
    out += [("high_permille", dict(flags=1, high_permille=1001)), ("low_permille", dict(flags=1, low_permille=500, high_permille=500)),
            ("low_permille", dict(flags=1, low_permille=700, high_permille=300))]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("devices", (None, [0, 0]))
def test_gpu_refusals(cr, hdr, rvs, devices):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    INVALID = _lib.CRT_ERR_INVALID
    assert L.crt_display(None, 1.0, None, 1) == INVALID and b"null scene" in L.crt_last_error()
    assert L.crt_display_reset(None) == INVALID and b"null scene" in L.crt_last_error()
    scene = hdr_scene(cr, hdr, rvs, before=None if devices is None else (lambda sc: sc.set_devices(devices)))
    try:
        h = scene._h
        rgba = np.zeros((H, W, 4), np.uint8)
        hist = np.zeros(256, np.uint32)
        st = _lib.crt_display_state()
        ptr = C.c_void_p()
        # before any successful crt_display
        for rc in (L.crt_read_display(h, rgba.ctypes.data_as(C.c_void_p), rgba.size), L.crt_display_device(h, C.byref(ptr)),
                   L.crt_display_get_state(h, C.byref(st)), L.crt_read_display_histogram(h, hist.ctypes.data_as(C.c_void_p))):
            assert rc == INVALID and b"no crt_display call" in L.crt_last_error()
        for source, text in ((1, b"no crt_denoise call has succeeded"), (2, b"no crt_temporal call has succeeded")):
            assert L.crt_display(h, 1.0, C.byref(raw_params(source=source)), 1) == INVALID and text in L.crt_last_error()
        assert L.crt_read_display(h, rgba.ctypes.data_as(C.c_void_p), rgba.size) == INVALID                # still none has succeeded
        scene.display(INV, curve="aces", exposure=0.75)
        assert L.crt_read_display_histogram(h, hist.ctypes.data_as(C.c_void_p)) == INVALID and b"metered" in L.crt_last_error()
        want = scene.display(INV, curve="aces", auto=True, adapt=0.5)
        state = scene.display_state()
        bins = scene.display_histogram()

        def unchanged(what):
            now = scene.display_state()
            assert {k: bits_of(v) for k, v in now.items()} == {k: bits_of(v) for k, v in state.items()}, what
            assert np.array_equal(scene.read_display(), want) and np.array_equal(scene.display_histogram(), bins), what

        for inv in (float("nan"), float("inf"), 0.0, -1.0):
            assert L.crt_display(h, inv, None, 1) == INVALID and b"inv_count" in L.crt_last_error(), inv
            unchanged(inv)
        for field, kw in refusals():
            assert L.crt_display(h, 1.0, C.byref(raw_params(**kw)), 1) == INVALID, (field, kw)
            assert field.encode() in L.crt_last_error(), (field, kw, L.crt_last_error())
            unchanged((field, kw))
        # with AUTO unset the meter's fields are not looked at
        assert L.crt_display(h, float(INV), C.byref(raw_params(curve=2, exposure=0.75, key=float("nan"), adapt=7.0, low_permille=9, high_permille=3)), 1) == 0
        assert L.crt_read_display(h, rgba.ctypes.data_as(C.c_void_p), rgba.size - 4) == INVALID and b"n_bytes" in L.crt_last_error()
        assert L.crt_read_display(h, None, rgba.size) == INVALID and L.crt_display_device(h, None) == INVALID
        assert L.crt_display_get_state(h, None) == INVALID and L.crt_read_display_histogram(h, None) == INVALID
    finally:
        scene.close()
