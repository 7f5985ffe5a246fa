"""crt_bloom (include/crt.h) against tests/bloom_ref.py: the bits of the bloomed image, its resolve and its display, always
on the source image read back from the device.  The CPU half holds bloom_ref to facts that need no device: level counts, a constant image,
a threshold above everything, the mass of a dyadic impulse, mirror symmetry where every level is even."""
import ctypes as C
import itertools

import numpy as np
import pytest

import bloom_ref as br
import display_ref as dr
import integrator_ref as ir

f32 = np.float32
SIZES = ((37, 23), (44, 28))     # odd and even; five levels and a 2 x 1 last level each
FRAMES = 4
INV = f32(1.0 / FRAMES)
# levels, conserve, threshold, clamp, inv_count: every combination
COMBOS = list(itertools.product((1, 3, 8), (True, False), (0.0, 1.0), (0.0, 50.0), (0.25, 7.0)))


def bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def params_of(combo, source="sum"):
    levels, conserve, threshold, clamp, _ = combo
    return br.Params(source=source, levels=levels, conserve=conserve, threshold=threshold, clamp=clamp, scatter=0.6, strength=0.3 if conserve else 0.8)


def same_bits(got, want, what):
    bad = np.nonzero((bits(got) != bits(want)).any(-1))
    assert bad[0].size == 0, (what, bad[0].size, list(zip(*bad))[:3], got[bad][:3], want[bad][:3])


# ---------------------------------------------------------------------------------------------- CPU: the reference itself

def test_level_counts():
    table = {(1, 1): (0, 0, 0), (1, 9): (0, 0, 0), (2, 2): (1, 1, 1), (3, 5): (1, 2, 2), (37, 23): (1, 3, 5), (44, 28): (1, 3, 5), (64, 64): (1, 3, 6)}
    for (w, h), want in table.items():
        assert tuple(br.level_count(w, h, levels) for levels in (1, 3, 8)) == want, (w, h)
    assert br.level_sizes(44, 28, 8)[-1] == (2, 1) and br.level_sizes(37, 23, 8)[-1] == (2, 1)
    assert br.level_sizes(257, 3, 8) == [(257, 3), (129, 2), (65, 1)]


def test_a_constant_image_comes_back():
    image = np.full((23, 37, 3), 0.5, f32)
    out = br.bloom(image, f32(1.0), br.Params(levels=8, conserve=True, scatter=0.5, strength=0.25))
    assert np.array_equal(bits(out), bits(image))


def test_a_threshold_above_every_pixel_adds_nothing():
    rng = np.random.default_rng(30)
    image = (4.0 * rng.random((23, 37, 3))).astype(f32)
    out = br.bloom(image, f32(1.0), br.Params(levels=8, conserve=False, threshold=100.0, strength=0.8))
    assert np.array_equal(bits(out), bits(image))


def impulse_image(width=32, height=32, at=(17, 13)):
    image = np.zeros((height, width, 3), f32)
    image[at[1], at[0]] = (2.0 ** 20, 2.0 ** 19, 2.0 ** 18)
    return image


IMPULSE = dict(levels=1, conserve=True, scatter=0.5, strength=0.5)


def test_a_dyadic_impulse_keeps_its_mass():
    image = impulse_image()
    out = br.bloom(image, f32(1.0), br.Params(**IMPULSE))
    assert np.array_equal(out.astype(np.float64).sum((0, 1)), image.astype(np.float64).sum((0, 1)))
    assert int((out != 0).any(-1).sum()) == 36


def test_mirrors_where_every_level_is_even():
    rng = np.random.default_rng(31)
    image = (4.0 * rng.random((64, 64, 3))).astype(f32)
    image[9, 50] = 400.0
    p = br.Params(levels=6, conserve=False, threshold=1.0, clamp=50.0)
    out = br.bloom(image, f32(1.0), p)
    assert np.array_equal(bits(br.bloom(image[:, ::-1], f32(1.0), p)), bits(out[:, ::-1]))
    assert np.array_equal(bits(br.bloom(image[::-1], f32(1.0), p)), bits(out[::-1]))
    assert not np.array_equal(bits(out), bits(image))


def test_no_level_returns_the_input():
    rng = np.random.default_rng(32)
    for shape in ((1, 1, 3), (9, 1, 3), (1, 9, 3)):
        image = rng.random(shape).astype(f32)
        assert np.array_equal(bits(br.bloom(image, f32(0.25), br.Params(levels=8))), bits(F32(image * f32(0.25))))
        assert np.array_equal(bits(br.bloom(image, f32(0.25), br.Params(source="denoised", levels=8))), bits(image))


def F32(x):
    return np.asarray(x, f32)


def test_abi_of_the_params():
    from caitlynrenderer_amd import _lib
    assert C.sizeof(_lib.crt_bloom_params) == 32
    for name in ("crt_bloom", "crt_read_bloom", "crt_bloom_device", "crt_resolve_bloom", "crt_resolve_bloom_device", "crt_display_bloom"):
        assert name in _lib.SYMBOLS and getattr(_lib.lib(), name) is not None


# ---------------------------------------------------------------------------------------------- GPU

@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def hdr(cr):
    """§28's cube on its ground quad under test_display's environment: (mesh, SceneData, camera, environment)"""
    from test_display import hdr_env
    from test_environment import cube_quad_scene
    mesh, cam = cube_quad_scene(cr)
    return mesh, cr.SceneData.build(mesh, cam), cam, hdr_env()


def hdr_scene(cr, hdr, rvs, size, before=None):
    from test_display import hdr_scene as make
    return make(cr, hdr, rvs, before=before, width=size[0], height=size[1])


def check_bloom(scene, image, combo, source="sum", what=None):
    """one bloom() against the reference on `image`; returns the image read back"""
    p = params_of(combo, source)
    inv = f32(combo[4])
    scene.bloom(inv, **p.kwargs())
    got = scene.read_bloom()
    same_bits(got, br.bloom(image, inv, p), (what, combo))
    return got


def check_outputs(scene, bloomed):
    """the bloomed image's resolve, and its display: a metered call and a manual one after it"""
    assert np.array_equal(scene.resolve_bloom(), ir.resolve_ref(bloomed, f32(1.0)))
    meter = dr.Meter()
    scene.display_reset()
    for p in (dr.Params(source="denoised", curve="aces", auto=True, adapt=0.5), dr.Params(source="denoised", curve="reinhard", exposure=0.5, white=2.0)):
        want, state, hist = dr.display(bloomed, f32(1.0), p, meter)            # "denoised": the image as it is
        kw = p.kwargs()
        kw["source"] = "bloom"
        got = scene.display(**kw)
        st = scene.display_state()
        assert (st["counted"], st["q"], st["calls"]) == (state["counted"], state["q"], state["calls"]), (st, state)
        assert bits(st["metered"]) == bits(state["metered"]) and bits(st["exposure"]) == bits(state["exposure"]), (st, state)
        if p.auto:
            assert scene.display_histogram().tolist() == hist
        assert np.array_equal(got, want)
    assert np.array_equal(bits(scene.read_bloom()), bits(bloomed))


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_gpu_hdr_sum(cr, hdr, rvs, size):
    scene = hdr_scene(cr, hdr, rvs, size)
    try:
        image = scene.read_sum()
        lum = br.luminance(F32(image * f32(0.25)))
        assert float(lum.min()) < 1.0 < float(lum.max()) and float(br.luminance(F32(image * f32(7.0))).max()) > 50.0     # the threshold cuts, and the clamp at inv_count 7
        seen = set()
        for i, combo in enumerate(COMBOS):
            got = check_bloom(scene, image, combo, what=size)
            seen.add(got.tobytes())
            if i % 7 == 0:
                check_outputs(scene, got)
        assert len(seen) == len(COMBOS) * 3 // 4           # every field acts; at inv_count 0.25 no luminance reaches the clamp of 50
        assert np.array_equal(bits(scene.read_sum()), bits(image))
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES)
def test_gpu_sources(cr, hdr, rvs, size):
    from caitlynrenderer_amd.scene import AOV_ALL
    scene = hdr_scene(cr, hdr, rvs, size)
    try:
        scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
        scene.denoise(INV, passes=3)
        scene.temporal(INV, source="sum")
        for source, read in (("denoised", scene.read_denoised), ("temporal", scene.read_temporal)):
            image = read()
            assert float(image.max()) > 0.0
            by_inv = {}
            for i, combo in enumerate(COMBOS):
                got = check_bloom(scene, image, combo, source, what=(size, source))
                by_inv.setdefault(combo[:4], []).append(got.tobytes())
                if i % 16 == 0:
                    check_outputs(scene, got)
            assert all(len(v) == 2 and v[0] == v[1] for v in by_inv.values())          # inv_count is checked and then ignored
            assert np.array_equal(bits(read()), bits(image))
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_many_workgroups(cr, hdr, rvs):
    """301 x 233: every level down to the fourth spans several workgroups, and the last column and row of workgroups are partly outside"""
    scene = hdr_scene(cr, hdr, rvs[:2], (301, 233))
    try:
        image = scene.read_sum()
        for combo in ((8, True, 0.0, 0.0, 0.5), (8, False, 1.0, 50.0, 0.5), (2, True, 0.0, 50.0, 0.5)):
            got = check_bloom(scene, image, combo, what="301 x 233")
        assert np.array_equal(scene.resolve_bloom(), ir.resolve_ref(got, f32(1.0)))
    finally:
        scene.close()


@pytest.mark.gpu
@pytest.mark.parametrize("size", ((1, 1), (257, 3)))
def test_gpu_small_frames(cr, hdr, rvs, size):
    scene = hdr_scene(cr, hdr, rvs, size)
    try:
        image = scene.read_sum()
        assert br.level_count(size[0], size[1], 8) == (0 if size == (1, 1) else 2)
        for combo in ((8, True, 0.0, 0.0, 0.25), (8, False, 1.0, 50.0, 7.0), (1, False, 0.0, 0.0, 0.25)):
            got = check_bloom(scene, image, combo, what=size)
            if size == (1, 1):
                assert np.array_equal(bits(got), bits(F32(image * f32(combo[4]))))
        check_outputs(scene, got)
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_two_devices_and_a_shard(cr, hdr, rvs):
    from caitlynrenderer_amd import _lib
    scene = hdr_scene(cr, hdr, rvs, SIZES[1], before=lambda sc: sc.set_devices([0, 0]))
    try:
        image = scene.read_sum()
        assert image.any()
        for combo in (COMBOS[0], COMBOS[-1], (3, False, 1.0, 0.0, 0.25)):
            got = check_bloom(scene, image, combo, what="two devices")
        check_outputs(scene, got)
    finally:
        scene.close()
    scene = hdr_scene(cr, hdr, rvs, SIZES[1], before=lambda sc: sc.set_shard(0, 2, 8))
    try:
        with pytest.raises(_lib.CrtError, match="shard"):
            scene.bloom(INV)
        with pytest.raises(_lib.CrtError, match="no crt_bloom call has succeeded"):
            scene.read_bloom()
    finally:
        scene.close()


def wall_scene(cr, px, cols, rows):
    from test_integrator_ref import emitter_wall
    mesh, cam, width, height = emitter_wall(cr, px, cols, rows)
    scene = cr.Scene(cr.SceneData.build(mesh, cam), width, height, 1)
    try:
        scene.render_frame(0.37, 0.61)
    except Exception:
        scene.close()
        raise
    return scene


@pytest.mark.gpu
def test_gpu_exact_floats_the_impulse(cr):
    px = np.zeros((11 * 11, 3), f32)
    px[6 * 11 + 5] = (2.0 ** 20, 2.0 ** 19, 2.0 ** 18)
    scene = wall_scene(cr, px, 11, 11)
    try:
        image = scene.read_sum()
        assert int((image != 0).any(-1).sum()) == 9 and set(np.unique(image).tolist()) == {0.0, 2.0 ** 18, 2.0 ** 19, 2.0 ** 20}
        p = br.Params(**IMPULSE)
        scene.bloom(f32(1.0), **p.kwargs())
        got = scene.read_bloom()
        same_bits(got, br.bloom(image, f32(1.0), p), "impulse")
        assert np.array_equal(got.astype(np.float64).sum((0, 1)), image.astype(np.float64).sum((0, 1)))
        assert int((got != 0).any(-1).sum()) > 9
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_exact_floats_the_hostile_wall(cr):
    rng = np.random.default_rng(33)
    px = (0.1 + 2.0 * rng.random((8 * 6, 3))).astype(f32)
    for q, v in ((9, np.inf), (14, np.nan), (20, 1e38), (27, 0.0), (30, -1.0), (37, 1e-41)):
        px[q] = v
    scene = wall_scene(cr, px, 8, 6)
    try:
        image = scene.read_sum()
        assert np.isinf(image).any() and np.isnan(image).any() and (image == f32(1e38)).any() and (image == f32(1e-41)).any() and (image < 0).any()
        for conserve, threshold, clamp in itertools.product((True, False), (0.0, 1.0), (0.0, 50.0)):
            p = br.Params(levels=1, conserve=conserve, threshold=threshold, clamp=clamp, scatter=0.5, strength=0.5)
            scene.bloom(f32(1.0), **p.kwargs())
            got, want = scene.read_bloom(), br.bloom(image, f32(1.0), p)
            assert np.array_equal(np.isnan(got), np.isnan(want)), (conserve, threshold, clamp)
            ok = ~np.isnan(want)
            assert np.array_equal(bits(got)[ok], bits(want)[ok]), (conserve, threshold, clamp)
            # the NaNs come from the inf and the NaN quad; the clamp keeps 1e38 from overflowing in the filter, without it 3 * (2e38) is inf
            assert np.isnan(want).any() and (clamp != 0.0 or np.isinf(want).any())
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_the_buffers_stay(cr, hdr, rvs):
    from test_denoise import device_bytes_at, device_bytes_in_use
    size = SIZES[0]
    scene = hdr_scene(cr, hdr, rvs, size)
    try:
        image = scene.read_sum()
        first = check_bloom(scene, image, COMBOS[0])
        p, q = scene.bloom_device(), scene.resolve_bloom_device()
        assert p and q and np.array_equal(device_bytes_at(p, size[0] * size[1] * 12), np.ascontiguousarray(first).view(np.uint8).reshape(-1))
        assert np.array_equal(device_bytes_at(q, size[0] * size[1] * 4), ir.resolve_ref(first, f32(1.0)).reshape(-1))
        scene.display(source="bloom")
        scene.read_bloom()
        scene.resolve_bloom()
        in_use = device_bytes_in_use()
        second = check_bloom(scene, image, COMBOS[-1])
        assert not np.array_equal(bits(first), bits(second))
        assert scene.bloom_device() == p and scene.resolve_bloom_device() == q
        scene.reset()
        scene.render_frames(rvs[:2])
        check_bloom(scene, scene.read_sum(), (8, True, 0.0, 50.0, 0.5))
        scene.display(source="bloom", curve="aces", auto=True)
        assert scene.bloom_device() == p and scene.resolve_bloom_device() == q and device_bytes_in_use() == in_use
    finally:
        scene.close()


@pytest.mark.gpu
def test_gpu_ordering(cr, hdr, rvs):
    _, data, cam, env = hdr
    from test_display import set_env
    out = []
    for sync in (True, False):
        scene = cr.Scene(data, 44, 28, 3)
        try:
            scene.update(cam)
            set_env(scene, env)
            scene.render_frames(rvs, sync=sync)
            scene.bloom(INV, levels=8, sync=sync)
            scene.display(source="bloom", curve="aces", auto=True, sync=sync)
            scene.sync()
            out.append((scene.read_bloom(), scene.read_display()))
        finally:
            scene.close()
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(out[0][1], out[1][1])


@pytest.mark.gpu
def test_gpu_bloom_leaves_everything_alone(cr, hdr, rvs):
    from caitlynrenderer_amd.scene import AOV_ALL
    from test_denoise import device_bytes_at
    size = SIZES[1]
    n_rgba = size[0] * size[1] * 4
    scene = hdr_scene(cr, hdr, rvs, size)
    try:
        scene.render_aov(rvs[0][0], rvs[0][1], AOV_ALL)
        scene.denoise(INV, passes=2)
        scene.temporal(INV, source="sum")
        scene.render_frame(*rvs[0])
        scene.frame_count = FRAMES + 1
        scene.display(INV, curve="aces", auto=True)
        pointers = (scene.resolve_device(INV), scene.resolve_denoised_device(), scene.resolve_temporal_device(), scene.display_device())

        def everything():
            return (scene.read_packed().tobytes(), [np.ascontiguousarray(scene.read_aov(1 << k)).tobytes() for k in range(5)], scene.frame_stats(),
                    scene.launch_info(), scene.frame_count, scene.read_denoised().tobytes(), scene.read_temporal().tobytes(),
                    [device_bytes_at(p, n_rgba).tobytes() for p in pointers], {k: bits(v).tolist() for k, v in scene.display_state().items()})

        before = everything()
        for source in br.SOURCES:
            scene.bloom(INV, source=source, levels=8, threshold=0.5)
            scene.resolve_bloom()
        assert everything() == before
        scene.render_frame(*rvs[0])
        assert scene.launch_info() == before[3]
    finally:
        scene.close()


def raw_params(**kw):
    from caitlynrenderer_amd._lib import crt_bloom_params
    p = crt_bloom_params()
    p.source, p.levels, p.flags, p.threshold, p.clamp, p.scatter, p.strength, p.reserved = 0, 6, 1, 0.0, 0.0, 0.7, 0.05, 0
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def refusals():
    nan, inf = float("nan"), float("inf")
    out = [("source", dict(source=3)), ("flag", dict(flags=2)), ("flag", dict(flags=0x80000001)), ("levels", dict(levels=0)), ("levels", dict(levels=9)),
           ("reserved", dict(reserved=1))]
    out += [("threshold", dict(threshold=v)) for v in (nan, inf, -0.5, 2e6)]
    out += [("clamp", dict(clamp=v)) for v in (nan, inf, -1.0, 1e-7, 1e10)]
    out += [("scatter", dict(scatter=v)) for v in (nan, inf, -0.1, 1.5)]
    out += [("strength", dict(strength=v)) for v in (nan, inf, -0.1, 1.5)]
    out += [("strength", dict(flags=0, strength=v)) for v in (nan, inf, -0.1, 2e3)]
    return out


@pytest.mark.gpu
def test_gpu_refusals(cr, hdr, rvs):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    INVALID = _lib.CRT_ERR_INVALID
    assert L.crt_bloom(None, 1.0, None, 1) == INVALID and b"null scene" in L.crt_last_error()
    assert L.crt_display_bloom(None, None, 1) == INVALID and b"null scene" in L.crt_last_error()
    W, H = SIZES[1]
    scene = hdr_scene(cr, hdr, rvs, SIZES[1])
    try:
        h = scene._h
        rgb, rgba, ptr = np.zeros((H, W, 3), f32), np.zeros((H, W, 4), np.uint8), C.c_void_p()
        as_p = lambda a: a.ctypes.data_as(C.c_void_p)
        for call in (lambda: L.crt_read_bloom(h, as_p(rgb), rgb.size), lambda: L.crt_bloom_device(h, C.byref(ptr)), lambda: L.crt_resolve_bloom(h, as_p(rgba), rgba.size),
                     lambda: L.crt_resolve_bloom_device(h, C.byref(ptr), 1), lambda: L.crt_display_bloom(h, None, 1)):
            assert call() == INVALID and b"no crt_bloom call has succeeded" in L.crt_last_error()
        for source, text in ((1, b"no crt_denoise call has succeeded"), (2, b"no crt_temporal call has succeeded")):
            assert L.crt_bloom(h, 1.0, C.byref(raw_params(source=source)), 1) == INVALID and text in L.crt_last_error()
        assert L.crt_read_bloom(h, as_p(rgb), rgb.size) == INVALID                           # still none has succeeded
        assert L.crt_bloom(h, float(INV), None, 1) == 0                                     # NULL params: the header's defaults
        want = scene.read_bloom()
        same_bits(want, br.bloom(scene.read_sum(), INV, br.Params()), "NULL params")
        scene.bloom(INV)                                                                     # and the binding's
        assert np.array_equal(bits(scene.read_bloom()), bits(want))

        def unchanged(what):
            assert np.array_equal(bits(scene.read_bloom()), bits(want)), what

        for inv in (float("nan"), float("inf"), 0.0, -1.0):
            assert L.crt_bloom(h, inv, None, 1) == INVALID and b"inv_count" in L.crt_last_error(), inv
            assert L.crt_bloom(h, inv, C.byref(raw_params(source=1)), 1) == INVALID and b"inv_count" in L.crt_last_error(), inv
            unchanged(inv)
        for field, kw in refusals():
            assert L.crt_bloom(h, 1.0, C.byref(raw_params(**kw)), 1) == INVALID, (field, kw)
            assert field.encode() in L.crt_last_error(), (field, kw, L.crt_last_error())
            unchanged((field, kw))
        assert L.crt_bloom(h, 1.0, C.byref(raw_params(flags=0, strength=1.5)), 1) == 0      # additive: above 1 is in range
        assert L.crt_bloom(h, float(INV), None, 1) == 0
        unchanged("the defaults again")
        # wrong sizes and null arguments
        assert L.crt_read_bloom(h, as_p(rgb), rgb.size - 3) == INVALID and b"n_floats" in L.crt_last_error()
        assert L.crt_resolve_bloom(h, as_p(rgba), rgba.size - 4) == INVALID and b"n_bytes" in L.crt_last_error()
        assert L.crt_read_bloom(h, None, rgb.size) == INVALID and L.crt_bloom_device(h, None) == INVALID
        assert L.crt_resolve_bloom(h, None, rgba.size) == INVALID and L.crt_resolve_bloom_device(h, None, 1) == INVALID
        # crt_display_bloom: crt_display's refusals, and a source that names nothing
        from test_display import raw_params as display_params, refusals as display_refusals
        shown = scene.display(source="bloom", curve="aces", auto=True)
        for field, kw in display_refusals():
            if field == "source":
                continue
            assert L.crt_display_bloom(h, C.byref(display_params(**kw)), 1) == INVALID, (field, kw)
            assert field.encode() in L.crt_last_error() and b"crt_display_bloom" in L.crt_last_error(), (field, kw, L.crt_last_error())
        for source in (1, 2, 3):
            assert L.crt_display_bloom(h, C.byref(display_params(source=source)), 1) == INVALID and b"source" in L.crt_last_error()
        assert np.array_equal(scene.read_display(), shown)
        unchanged("after the display refusals")
    finally:
        scene.close()
