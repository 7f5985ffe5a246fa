"""The path integrator (`k_segment` and its shell) and `k_resolve` held to tests/integrator_ref.py: a numpy restatement written from
Shader/path_trace.fs and DESIGN.md §3 that shares no code with oracle/oracle.c or the library (DESIGN.md "The integrator as tested").

CPU cases: the reference's own arithmetic (an exact fma, the pinned sine and cosine), the reference against the C oracle (brute force and
BVH8) by bits, its primary rays, the resolve at every byte change.  GPU cases: the HIP frame path against the reference directly — the
oracle is not involved — sums as uint32 words, ray counts against the reference's census, and Scene.resolve() against resolve_ref.

All comparisons are exact.  The only numbers are conditions on the inputs: every branch of scene (d) is taken by at least 20
pixel-samples, and the resolve set straddles at least 250 of the 255 byte changes in every channel."""
import ctypes
import ctypes.util
import fractions
import math

import numpy as np
import pytest

import integrator_ref as ir

W, H = 44, 28               # no multiple of the 8-, 16- or 64-pixel tiles; W != H so the aspect factor matters
FRAMES = 4
MAX_DEPTH = 4
SCENES = ("cornell", "tess8", "textured", "hand", "hand_unlit")
MIN_BRANCH = 20


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---------------------------------------------------------------------------------------------- scene (d), built by hand

def _quad(p, a, b):
    """two triangles of the parallelogram p, p + a, p + a + b, p + b"""
    p, a, b = np.asarray(p, np.float32), np.asarray(a, np.float32), np.asarray(b, np.float32)
    return [(p, p + a, p + a + b), (p, p + a + b, p + b)]


def hand_made_mesh(cr, lit=True, mirror=True):
    """Scene (d): 17 triangles in front of a camera at (0, 0.5, 0) that looks along +z.

      back wall z = 10, left half with vertex normals (0, 0, 1) (they face away: flipped to (0, 0, -1), the singular arm of onb, and NEE is
        refused on original_n where the flipped normal would accept), right half with (0, 0, -1)
      floor y = -3 with a FLAT integer normal (0, 1, 0) (vn.w == 0)
      an occluder y = -1 under light A with vertex normals of length 2; it shadows the floor
      a Mirror patch just in front of the right wall half; it shows light C, which hangs behind the camera
      light A  y = 2.9 facing down, seen directly above the wall's top edge
      light B  z = 8 facing the camera, two units in front of the wall: the wall's bounce rays reach its back side, and the right wall
               half, which lies behind its plane, is refused its light (cos_light >= 0)
      light C  z = -2 facing +z, behind the camera
      light D  one triangle at z = 9 with the flat normal (0, 0, 0): cos_incident == 0, no flip, cos_light == -0 <= 0, the pdf is
               -inf and the MIS weight 0 (the only way to cos_light <= 0: a face-forwarded normal gives cos_light > 0 on either side)
    Rays above the wall and beside it leave the scene at segment 0, bounce rays at later ones.
    lit=False is scene (e): the lights array empty — and, because crt_scene_create refuses an emissive material without its light, the
    four lamps turned into dark Lambert surfaces, D with the flat normal (0, 0, -1): with a zero normal a bounce would start ON the triangle
    (hit_point = o + d t + 0), where a hit at t = 0 is found by a brute force and culled by the tree walks' `exit > 0` box test — a matter
    of the walks, not of the integrator.  mirror=False turns the Mirror patch into a Lambert one (the BVH2 frame mode refuses
    Mirror materials)."""
    normals = np.array([[0, 0, 1], [0, 0, -1], [0, 2, 0], [0, -1, 0]], np.float32)
    tris, mats, lights = [], [], []
    verts = []

    def material(albedo, kind=0.0, emission=None):
        m = np.full(16, -1.0, np.float32)
        m[0:3], m[3] = albedo, kind
        m[4:7], m[7] = (0, 0, 0), -1.0
        m[8:12] = 0.0
        if emission is not None and lit:
            m[4:7], m[7] = emission, float(len(lights))
        mats.append(m)
        return len(mats) - 1

    def add(tri_list, mtl, vn=None, flat=None):
        for t in tri_list:
            i = len(verts)
            verts.extend(t)
            row = [i, i + 1, i + 2, mtl] + ([vn, vn, vn, 1] if flat is None else list(flat) + [0]) + [-1, -1, -1, 0]
            tris.append(row)

    def lamp(tri_list, emission, normal, vn=None, flat=None):
        for t in tri_list:
            mtl = material((0.0, 0.0, 0.0), emission=emission)
            if lit:
                u, v = t[1] - t[0], t[2] - t[0]
                area = float(np.linalg.norm(np.cross(u.astype(np.float64), v.astype(np.float64))))       # |u x v|, as the loader has it
                lights.append(np.concatenate([t[0], u, v, np.asarray(normal, np.float32), np.asarray(emission, np.float32),
                                              [area, 0.0, 0.0]]).astype(np.float32))
            add([t], mtl, vn, flat)

    add(_quad((-4, -3, 10), (4, 0, 0), (0, 6, 0)), material((0.7, 0.7, 0.7)), vn=0)
    add(_quad((0, -3, 10), (4, 0, 0), (0, 6, 0)), material((0.6, 0.7, 0.3)), vn=1)
    add(_quad((-4, -3, 2), (8, 0, 0), (0, 0, 8)), material((0.5, 0.5, 0.6)), flat=(0, 1, 0))
    add(_quad((-1.5, -1, 4.5), (3, 0, 0), (0, 0, 3)), material((0.7, 0.3, 0.3)), vn=2)
    add(_quad((1, -1, 9.9), (2, 0, 0), (0, 2, 0)), material((0.8, 0.8, 0.8), kind=1.0 if mirror else 0.0), vn=1)
    lamp(_quad((-1, 2.9, 5), (2, 0, 0), (0, 0, 2)), (6.0, 6.0, 5.0), (0, -1, 0), vn=3)
    lamp(_quad((-3.5, -1, 8), (3, 0, 0), (0, 3, 0)), (3.0, 2.0, 1.0), (0, 0, -1), vn=1)
    lamp(_quad((-6, -4, -2), (12, 0, 0), (0, 8, 0)), (0.5, 0.5, 0.7), (0, 0, 1), vn=0)
    lamp([tuple(np.asarray(p, np.float32) for p in ((0.2, -2.8, 9), (3.8, -2.8, 9), (2, -1.2, 9)))], (1.0, 2.0, 1.0), (0, 0, -1), flat=(0, 0, 0) if lit else (0, 0, -1))
    L = np.array(lights, np.float32).reshape(-1, 18)
    if L.shape[0]:
        L[:, 16] = L[:, 15] / L[:, 15].sum(dtype=np.float32)                      # pdf = area / sum of the areas
    mesh = cr.Mesh(np.array(verts, np.float32), normals, np.zeros((0, 2), np.float32), np.array(tris, np.int32), np.array(mats, np.float32), L)
    return mesh, cr.Camera((0.0, 0.5, 0.0), (0.0, 0.5, 1.0), 60.0)


# ---------------------------------------------------------------------------------------------- shared, computed once

@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(FRAMES)]


@pytest.fixture(scope="module")
def cases(cr, cornell, cornell_data, tess8, textured):
    """name -> (mesh, SceneData, camera)"""
    out = {"cornell": (cornell[0], cornell_data, cornell[1]), "tess8": (tess8[0], tess8[1], cornell[1]),
           "textured": (textured[0], textured[1], textured[2])}
    for name, kw in (("hand", {}), ("hand_unlit", {"lit": False}), ("hand_lambert", {"mirror": False})):
        mesh, cam = hand_made_mesh(cr, **kw)
        out[name] = (mesh, cr.SceneData.build(mesh, cam), cam)
    return out


class _Lazy(dict):
    def __init__(self, make):
        super().__init__()
        self.make = make

    def __missing__(self, key):
        self[key] = self.make(key)
        return self[key]


@pytest.fixture(scope="module")
def reference(cases, rvs):
    """name -> (sums[depth - 1], per-frame census [frame][depth - 1], census[depth - 1] over the 4 frames): one run at MAX_DEPTH gives every
    shorter depth, because a path cut at k segments holds the L of k passes"""
    def make(name):
        mesh, _, cam = cases[name]
        sums, _, total, per_frame = ir.render(ir.RefScene(mesh, cam, W, H), rvs, MAX_DEPTH)
        for s in sums:
            s.setflags(write=False)
        return sums, per_frame, total
    return _Lazy(make)


# ---------------------------------------------------------------------------------------------- the reference's own arithmetic

def _fraction_fma(a, b, c):
    """a * b + c exactly, rounded once to the nearest double, ties to even"""
    x = fractions.Fraction(a) * fractions.Fraction(b) + fractions.Fraction(c)
    if x == 0:
        return 0.0
    sign = -1 if x < 0 else 1
    x = abs(x)
    e = x.numerator.bit_length() - x.denominator.bit_length()
    if fractions.Fraction(2) ** e > x:
        e -= 1                                       # 2^e <= x < 2^(e + 1)
    q = x / fractions.Fraction(2) ** (e - 52)        # in [2^52, 2^53)
    n, rem = divmod(q.numerator, q.denominator)
    twice = 2 * rem
    if twice > q.denominator or (twice == q.denominator and n & 1):
        n += 1
    return sign * math.ldexp(n, e - 52)


def test_fma_is_exact():
    rng = np.random.default_rng(11)
    n = 2400
    a = rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))
    b = rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))
    c = rng.standard_normal(n) * np.exp2(rng.integers(-30, 30, n))
    # cancellation: c close to -a b, so the result is the product's rounding error and its neighbourhood
    c[:600] = -(a[:600] * b[:600]) * (1 + rng.integers(-3, 4, 600) * 2.0 ** -52)
    # near-ties: c an integer of 53 bits (its ulp is 1) and a b = 0.5 (1 + (i + j) 2^-30 + i j 2^-60): at, just above or just below the midpoint
    i, j = rng.integers(-3, 4, 600), rng.integers(-3, 4, 600)
    a[600:1200] = 1.0 + i * 2.0 ** -30
    b[600:1200] = 0.5 * (1.0 + j * 2.0 ** -30) * rng.choice([1.0, -1.0], 600)
    c[600:1200] = rng.integers(1 << 52, 1 << 53, 600).astype(np.float64) * rng.choice([1.0, -1.0], 600)
    # exact ties: a b = exactly half an ulp of c
    c[1200:1500] = rng.integers(1 << 52, 1 << 53, 300).astype(np.float64)
    a[1200:1500] = 0.5
    b[1200:1500] = rng.choice([1.0, -1.0, 3.0, -3.0], 300)
    # the shapes the pinned sine uses: k * -PI_n + x
    kk = np.rint(rng.uniform(-4e4, 4e4, 300))
    a[1500:1800], b[1500:1800], c[1500:1800] = kk, -ir._PI_1, kk * ir._PI_1 + rng.uniform(-1.6, 1.6, 300)
    got = ir.fma(a, b, c)
    want = np.array([_fraction_fma(float(x), float(y), float(z)) for x, y, z in zip(a, b, c)])
    assert n >= 2000 and np.array_equal(got.view(np.uint64), want.view(np.uint64)), int((got.view(np.uint64) != want.view(np.uint64)).sum())
    plain = a * b + c
    assert (plain != want).sum() > 300, "the triples must tell an fma from a multiply and an add"
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")                 # and libm's fma agrees with the Fraction value
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    assert all(libm.fma(float(x), float(y), float(z)) == w for x, y, z, w in zip(a, b, c, want))


def test_pinned_sine_and_cosine(vectors):
    x = vectors["sin_x"].view(np.float32)
    assert np.array_equal(bits(ir.pinned_sin(x)), vectors["sin_y"])
    assert np.array_equal(bits(ir.pinned_cos(x)), vectors["cos_y"])
    # and the arguments the integrator meets: the seed's dot products (up to a few thousand) and phi in [0, 2 pi)
    rng = np.random.default_rng(5)
    y = np.concatenate([x, rng.uniform(-6000, 6000, 4000).astype(np.float32), rng.uniform(0, 6.2831853, 4000).astype(np.float32)])
    assert np.abs(ir.pinned_sin(y).astype(np.float64) - np.sin(y.astype(np.float64))).max() <= 6e-8
    assert np.abs(ir.pinned_cos(y).astype(np.float64) - np.cos(y.astype(np.float64))).max() <= 6e-8


def test_rand_sequence(vectors, ob):
    rng = ir._Rng(np.float32([3.5, 10.5]), np.float32([7.5, 0.5]), 0.6591631, 0.910802)
    mine = np.stack([rng.draw(np.ones(2, bool)) for _ in range(16)])
    for col, (px, py) in enumerate(((3, 7), (10, 0))):
        assert np.array_equal(bits(mine[:, col]), bits(np.float32(ob.rand_sequence(px, py, 0.6591631, 0.910802, 16))))


# ---------------------------------------------------------------------------------------------- the reference against the oracle

@pytest.mark.parametrize("name", SCENES)
def test_primary_rays_equal_the_oracle(ob, cases, rvs, name):
    mesh, data, cam = cases[name]
    scene = ir.RefScene(mesh, cam, W, H)
    orc = ob.Oracle(data, W, H, 1, cam)
    for rx, ry in rvs:
        o, d, _, census = ir.primary_rays(scene, rx, ry, jitter=True)
        want = orc.primary_rays(rx, ry, jitter=True)
        assert np.array_equal(bits(d), bits(want["d"])) and np.array_equal(bits(o), bits(want["o"]))
        assert min(census.values()) > W * H // 4                       # both arms of each jitter component


@pytest.mark.parametrize("depth", (1, 2, 3, 4))
@pytest.mark.parametrize("name", SCENES)
def test_reference_equals_the_oracle(ob, cases, rvs, reference, name, depth):
    """Zero differing words in the sums after 4 frames, against the oracle's brute force and its BVH8 walk; ray counts too."""
    _, data, cam = cases[name]
    sums, per_frame, _ = reference[name]
    orc = ob.Oracle(data, W, H, depth, cam)
    for accel in (ob.BRUTE, ob.BVH8):
        acc = np.zeros((H, W, 3), np.float32)
        for f, (rx, ry) in enumerate(rvs):
            _, cnt = orc.render_frame(rx, ry, acc, accel=accel)
            assert (cnt[0], cnt[1]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), (accel, f)
        differing = int((bits(acc) != bits(sums[depth - 1])).sum())
        assert differing == 0, (name, depth, accel, differing)
    if name != "hand_unlit":
        assert sums[depth - 1].max() > 0.4


def test_hand_made_scene_takes_every_branch(reference):
    """The census of scene (d) in the reference alone, paths of 4 segments, 4 frames: no branch is tested emptily."""
    census = reference["hand"][2][MAX_DEPTH - 1]
    for key in ("onb_singular", "onb_regular", "emitter_direct", "emitter_after_bounce_front", "emitter_after_bounce_back",
                "emitter_cos_light_le_0", "nee_refused_cos_mtl_flipped_accepts", "nee_refused_cos_light", "shadow_occluded", "shadow_clear",
                "flat_normal_hit", "non_unit_normal_hit", "mirror_hit", "emitter_through_mirror", "miss_first", "miss_later",
                "jitter_x_low", "jitter_x_high", "jitter_y_low", "jitter_y_high"):
        assert census[key] >= MIN_BRANCH, (key, census)
    # at depth 3, the shader's own bound, the same holds
    c3 = reference["hand"][2][2]
    assert min(c3[k] for k in ("emitter_after_bounce_front", "emitter_after_bounce_back", "emitter_cos_light_le_0", "emitter_through_mirror",
                               "miss_later", "shadow_occluded")) >= MIN_BRANCH, c3
    unlit = reference["hand_unlit"][2][MAX_DEPTH - 1]
    assert unlit["shadow_rays"] == 0 and unlit["miss_later"] >= MIN_BRANCH and unlit["closest_rays"] > 3 * FRAMES * W * H // 2


def test_textured_scene_reaches_the_texture(reference):
    assert reference["textured"][2][2]["textured_hit"] >= 200


# ---------------------------------------------------------------------------------------------- resolve

def _byte(values, inv, channel, weights):
    px = np.float32(values)[:, None] * np.float32(weights)[None, :]
    return ir.resolve_ref(px.astype(np.float32), inv)[:, channel].astype(np.int64)


def _threshold_values(inv, channel, weights):
    """For each byte change j - 1 -> j (j = 1..255) of `channel` along the ray s * weights: 5 consecutive floats s around the smallest s
    whose byte reaches j, found by bisection on the float's bit pattern with resolve_ref itself."""
    j = np.arange(1, 256)
    lo = np.full(255, np.float32(1e-12).view(np.uint32), np.int64)            # byte 0
    hi = np.full(255, np.float32(1e6).view(np.uint32), np.int64)              # byte 255
    assert (_byte(lo.astype(np.uint32).view(np.float32), inv, channel, weights) == 0).all()
    assert (_byte(hi.astype(np.uint32).view(np.float32), inv, channel, weights) == 255).all()
    while (hi - lo > 1).any():
        mid = (lo + hi) // 2
        reached = _byte(mid.astype(np.uint32).view(np.float32), inv, channel, weights) >= j
        hi = np.where(reached, mid, hi)
        lo = np.where(reached, lo, mid)
    around = (hi[:, None] + np.arange(-2, 3)[None, :]).astype(np.uint32).view(np.float32)          # (255, 5)
    return around


def resolve_set(inv):
    """(n, 3) float32 sums: grey and coloured rays through every byte change, and the special values."""
    rows = []
    for channel, weights in ((0, (1, 1, 1)), (0, (1, 0.7, 0.4)), (1, (0.4, 1, 0.7)), (2, (0.7, 0.4, 1))):
        s = _threshold_values(inv, channel, weights).reshape(-1)
        rows.append(s[:, None] * np.float32(weights)[None, :])
    special = np.float32([0.0, -0.0, -1.5, 1e-41, np.inf, np.nan, 0.25, 3.0])
    rows.append(np.stack([special, special, special], -1))
    rows.append(np.stack([special, np.roll(special, 1), np.roll(special, 3)], -1))
    return np.concatenate(rows).astype(np.float32)


def straddled(px, rgba):
    """per channel: how many of the 255 byte changes have, among pixels whose values are consecutive floats, both sides present —
    counted simply as the byte values j for which both j - 1 and j occur"""
    return [len({int(b) for b in np.unique(rgba[:, c])} & {int(b) + 1 for b in np.unique(rgba[:, c])}) for c in range(3)]


@pytest.mark.parametrize("inv", (1.0, 1.0 / 3.0))
def test_resolve_ref_equals_the_oracle_at_every_byte_change(ob, inv):
    px = resolve_set(np.float32(inv))
    want = ir.resolve_ref(px, np.float32(inv))
    # the set is fine enough: around each threshold the 5 consecutive floats fall on both sides
    grey = _threshold_values(np.float32(inv), 0, (1, 1, 1))
    b = _byte(grey.reshape(-1), np.float32(inv), 0, (1, 1, 1)).reshape(255, 5)
    assert ((b.min(1) == np.arange(0, 255)) & (b.max(1) == np.arange(1, 256))).sum() >= 250
    assert min(straddled(px, want)) >= 250
    got = ob.resolve(px, np.float32(inv))
    assert np.array_equal(got, want), int((got != want).sum())
    assert (want[:, 3] == 255).all()
    specials = ir.resolve_ref(np.float32([[0.0, -0.0, -1.5], [1e-41, np.inf, np.nan], [np.nan, 1.0, 1.0]]), np.float32(inv))
    assert specials[0, :3].tolist() == [0, 0, 0] and specials[1, 0] == 0 and specials[1, 1] == 0 and specials[1, 2] == 0


def test_resolve_matches_output_shader_formula_exactly(ob):
    """tests/test_oracle.py::test_resolve_matches_output_shader_formula allows one 8-bit step against a float64 formula; through resolve_ref the
    same input compares exactly"""
    rng = np.random.default_rng(3)
    s = (rng.random((40, 30, 3)) * 6).astype(np.float32)
    assert np.array_equal(ob.resolve(s, 0.25), ir.resolve_ref(s, np.float32(0.25)))


# ---------------------------------------------------------------------------------------------- the GPU against the reference

def _render_and_check(cr, data, reference_entry, rvs, depth, options=(), one_call=False):
    sums, per_frame, total = reference_entry
    scene = cr.Scene(data, W, H, depth)
    try:
        for k, v in options:
            scene.set_option(k, v)
        if one_call:
            scene.render_frames(rvs)
            st = scene.frame_stats()                                   # a batched launch reports its totals
            assert (st["closest_rays"], st["any_rays"]) == (total[depth - 1]["closest_rays"], total[depth - 1]["shadow_rays"])
        else:
            for f, (rx, ry) in enumerate(rvs):
                scene.render_frame(rx, ry)
                st = scene.frame_stats()
                assert (st["closest_rays"], st["any_rays"]) == (per_frame[f][depth - 1]["closest_rays"], per_frame[f][depth - 1]["shadow_rays"]), f
        got = scene.read_sum()
        differing = int((bits(got) != bits(sums[depth - 1])).sum())
        assert differing == 0, differing
        scene.frame_count = len(rvs)
        rgba = scene.resolve()
        assert np.array_equal(rgba, ir.resolve_ref(got, np.float32(1.0 / len(rvs))))
        assert np.array_equal(rgba, ir.resolve_ref(sums[depth - 1], np.float32(1.0 / len(rvs))))
    finally:
        scene.close()


GPU_CASES = [(n, d) for n in ("cornell", "tess8", "textured", "hand_unlit") for d in (1, 3)] + [("hand", d) for d in (1, 2, 3, 4)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,depth", GPU_CASES)
def test_gpu_frames_equal_the_reference(cr, cases, rvs, reference, name, depth):
    """k_segment against integrator_ref directly: the sums after four render_frame calls as uint32 words, each frame's closest and shadow
    ray counts against the census, and the resolved bytes against resolve_ref"""
    _render_and_check(cr, cases[name][1], reference[name], rvs, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("variant", ("render_frames", "inplace_shadow_1", "inplace_shadow_0", "bvh2_frame_mode", "device_built_sah"))
def test_gpu_variants_equal_the_reference(cr, cases, rvs, reference, variant):
    """Scene (d), paths of 3 segments, once through each other way to the same frame"""
    name, data, kw = "hand", cases["hand"][1], {}
    if variant == "render_frames":
        kw = {"one_call": True}
    elif variant == "inplace_shadow_1":
        kw = {"options": (("inplace_shadow", 1),)}
    elif variant == "inplace_shadow_0":
        kw = {"options": (("inplace_shadow", 0),)}
    elif variant == "bvh2_frame_mode":
        name, kw = "hand_lambert", {"options": (("accel", 1),)}        # the BVH2 frame mode is the Lambert-only shader: the patch is Lambert
        data = cases[name][1]
    else:
        mesh, _, cam = cases["hand"]
        data = cr.SceneData.for_device_build(mesh, cam, "sah")
    _render_and_check(cr, data, reference[name], rvs, 3, **kw)


def emitter_wall(cr, px, cols, rows):
    """A wall of cols x rows emissive quads that fills the view of a camera looking along +z, quad q with emission px[q]: a one-segment
    frame's sum holds px[q] — 0 + 1 * emission — at every pixel whose ray meets quad q.  This is how arbitrary floats get into the packed
    sum that Scene.resolve() reads (crt_sum_device names an un-tiled COPY, rewritten by every read)."""
    n = cols * rows
    assert px.shape[0] <= n
    fov, dist = 60.0, 4.0
    width, height = 3 * cols, 3 * rows
    half_h = dist * math.tan(math.radians(fov) / 2)
    half_w = half_h * width / height
    verts, tris = [], []
    mats = np.full((n, 16), -1.0, np.float32)
    mats[:, 0:4] = 0.0
    mats[:, 8:12] = 0.0
    mats[:, 4:7] = 0.25
    mats[:px.shape[0], 4:7] = px
    mats[:, 7] = 0.0
    for r in range(rows):
        for c in range(cols):
            x0, x1 = half_w - 2 * half_w * c / cols, half_w - 2 * half_w * (c + 1) / cols
            y0, y1 = -half_h + 2 * half_h * r / rows, -half_h + 2 * half_h * (r + 1) / rows
            i = len(verts)
            verts += [(x0, y0, dist), (x1, y0, dist), (x1, y1, dist), (x0, y1, dist)]
            q = r * cols + c
            tris += [[i, i + 1, i + 2, q, 0, 0, 0, 1, -1, -1, -1, 0], [i, i + 2, i + 3, q, 0, 0, 0, 1, -1, -1, -1, 0]]
    light = np.float32([[0, 0, dist, 1, 0, 0, 0, 1, 0, 0, 0, -1, 1, 1, 1, 1, 1, 0]])
    mesh = cr.Mesh(np.float32(verts), np.float32([[0, 0, -1]]), np.zeros((0, 2), np.float32), np.int32(tris), mats, light)
    return mesh, cr.Camera((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fov), width, height


@pytest.mark.gpu
@pytest.mark.parametrize("inv", (1.0, 1.0 / 3.0))
def test_gpu_resolve_equals_resolve_ref_at_every_byte_change(cr, inv):
    """k_resolve against resolve_ref on the threshold set, carried into the device sum by a one-segment frame of a wall of emitters; the sum
    is read back first and THAT is resolved by the reference, so neither the packed layout nor the walk matters"""
    px = resolve_set(np.float32(inv))
    cols = 96
    rows = -(-px.shape[0] // cols)
    mesh, cam, width, height = emitter_wall(cr, px, cols, rows)
    scene = cr.Scene(cr.SceneData.build(mesh, cam), width, height, 1)
    try:
        scene.render_frame(0.37, 0.61)
        got = scene.read_sum()
        rgba = scene.resolve(np.float32(inv))
        want = ir.resolve_ref(got, np.float32(inv))
        assert np.array_equal(rgba, want), int((rgba != want).sum())
        assert min(straddled(got.reshape(-1, 3), want.reshape(-1, 4))) >= 250
        finite = np.isfinite(px).all(1) & (px != 0).all(1) & (np.abs(px) > 1e-30).all(1)
        seen = {r.tobytes() for r in bits(got).reshape(-1, 3)}
        assert all(r.tobytes() in seen for r in bits(px[finite])), "every finite value of the set reaches the sum"
    finally:
        scene.close()
