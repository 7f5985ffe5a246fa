"""The LEAN form of the one-pass last-segment builds (option lean_build): stack pushes without the overflow check on
a tree the create-time validator passed, the walks' vote ratio and group size as constants, no tile-cost clock,
and the RNG's sine from fewer double-precision-rate instructions.  Every operation that still runs is the one that ran before, so the
sums are held bit for bit: option on against option off against the CPU oracle.

Tessellated Cornell box n = 8 (1,922 triangles), four samples through one crt_render_frames call on a one-segment path: the form the
bench's step has.  64x48 fills its waves; 33x17 is no multiple of the 4x4 quadrant or of the tile, so part-filled waves and the
`lane < 16` add path run."""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = [(64, 48), (33, 17)]


@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(4)]


@pytest.fixture(scope="module")
def scenes(cr, cornell, tess8, textured):
    """kind -> (scene data, camera): Lambert (the headline's <WIDE> build), Disney materials (<MAT>), textured (<TEX,MAT>)"""
    from caitlynrenderer_amd.meshgen import tessellated_cornell, with_disney_materials
    cam = cornell[1]
    # the tessellation leaves the texcoord indices unset: every pair of triangles gets the fixture's pattern (uv beyond 1: the wrap runs)
    t8 = tessellated_cornell(textured[0], 8)
    tris = t8.triangles.copy()
    pair = np.arange(tris.shape[0]) // 2
    o = 4 * (pair % 2)
    odd = np.arange(tris.shape[0]) % 2
    tris[:, 8], tris[:, 9], tris[:, 10], tris[:, 11] = o, o + 1 + odd, o + 2 + odd, 0
    tex = cr.Mesh(t8.vertices, t8.normals, t8.texcoords, tris, t8.materials, t8.lights, t8.vertex_min)
    tex.albedo_textures = textured[0].albedo_textures
    return {"lambert": (tess8[1], cam),
            "disney": (cr.SceneData.build(tessellated_cornell(with_disney_materials(cornell[0]), 8), cam), cam),
            "textured": (cr.SceneData.build(tex, cam), cam)}


@pytest.fixture(scope="module")
def oracle_sums(ob, scenes, rvs):
    """(kind, w, h) -> the oracle's sum of the four frames, computed once"""
    out = {}
    for kind, (data, cam) in scenes.items():
        for w, h in SIZES:
            orc = ob.Oracle(data, w, h, 1, cam)
            ref = np.zeros((h, w, 3), np.float32)
            for rx, ry in rvs:
                orc.render_frame(rx, ry, ref, threads=8)
            out[kind, w, h] = ref
    return out


def _scene(cr, data, w, h, depth=1, prime=None):
    """prime: frames rendered before anything is checked — the first launch of a new view clocks its tiles (16-pixel tiles: every frame
    here has several) and that one launch is never LEAN (test_first_frame_of_a_view_measures_tile_costs_in_the_other_build)"""
    sc = cr.Scene(data, w, h, depth)
    sc.set_option("wide_first", 1)      # a Lambert scene's one-pass build is the 6-wave one, which a frame this small would not pick by itself
    if prime:
        sc.render_frames(prime)
        sc.reset()
    return sc


def _render(sc, rvs, lean, counting=0):
    sc.set_option("lean_build", lean)
    sc.set_option("count_visits", counting)
    sc.reset()
    sc.render_frames(rvs)
    return sc.read_sum(), sc.frame_stats()


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("kind", ["lambert", "disney", "textured"])
def test_frames_with_the_option_on_and_off_and_the_oracle(cr, scenes, oracle_sums, rvs, kind, size):
    w, h = size
    data, _ = scenes[kind]
    ref = oracle_sums[kind, w, h]
    sc = _scene(cr, data, w, h, prime=rvs)
    sums = {}
    for lean in (1, 0, 1):
        out, st = _render(sc, rvs, lean)
        info = sc.debug_launch_info()
        print(kind, size, "lean_build", lean, info, "last", sc.debug_last_build(), "lean", sc.debug_lean_build(), "max", float(out.max()),
              "differing words vs oracle", int((out.view(np.uint32) != ref.view(np.uint32)).sum()), "max |d|", float(np.abs(out - ref).max()))
        assert info["one_pass"] and info["samples"] == 4 and sc.debug_last_build(), (kind, size, lean)
        assert sc.debug_lean_build() == bool(lean), (kind, size, lean)
        assert st["stack_overflows"] == 0
        assert out.max() > 0
        sums[lean] = out
        assert np.array_equal(out.view(np.uint32), sums[1].view(np.uint32)), (kind, size, lean)
    assert np.array_equal(sums[1].view(np.uint32), sums[0].view(np.uint32)), (kind, size)
    assert np.array_equal(sums[1].view(np.uint32), ref.view(np.uint32)), (kind, size)
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["lambert", "textured"])
def test_counting_form_is_untouched(cr, scenes, oracle_sums, rvs, kind):
    """count_visits 2 counts in the timed launch form through the STATS builds, which have no LEAN form: the same build, the same
    counters and the same sum whatever the option says."""
    w, h = SIZES[0]
    sc = _scene(cr, scenes[kind][0], w, h, prime=rvs)
    got = {}
    for lean in (1, 0):
        out, st = _render(sc, rvs, lean, counting=2)
        print(kind, "lean_build", lean, sc.debug_launch_info(), st)
        assert sc.debug_launch_info()["one_pass"] and sc.debug_last_build() and not sc.debug_lean_build()
        assert st["nodes_closest"] > 0 and st["tris_closest"] > 0
        got[lean] = (out, st)
    assert got[1][1] == got[0][1]
    assert np.array_equal(got[1][0].view(np.uint32), got[0][0].view(np.uint32))
    assert np.array_equal(got[1][0].view(np.uint32), oracle_sums[kind, w, h].view(np.uint32))
    sc.close()


@pytest.mark.gpu
def test_launch_says_which_form_it_ran(cr, cornell, cornell_data, scenes, rvs):
    """The LEAN bit shows for a one-pass last-segment launch of the timed builds on a validated tree with the walk constants the form has
    compiled in, and for nothing else."""
    w, h = SIZES[0]
    data = scenes["lambert"][0]
    sc = _scene(cr, data, w, h, prime=rvs)
    _render(sc, rvs, 1)
    assert sc.debug_launch_info()["one_pass"] and sc.debug_last_build() and sc.debug_lean_build()
    want = sc.read_sum()
    for name, value, back in (("last_build", 0, 1), ("tri_min", 3, 2), ("lanes_per_ray", 1, 8), ("wave_samples", 0, 2)):
        sc.set_option(name, value)
        out, _ = _render(sc, rvs, 1)
        print(name, value, sc.debug_launch_info(), sc.debug_last_build(), sc.debug_lean_build())
        assert not sc.debug_lean_build(), name
        assert np.array_equal(out.view(np.uint32), want.view(np.uint32)), name
        sc.set_option(name, back)
    _render(sc, rvs, 1)
    assert sc.debug_lean_build()
    sc.render_frames(rvs[:1])                                     # one sample: the single-sample build
    assert not sc.debug_launch_info()["one_pass"] and not sc.debug_lean_build()
    sc.close()
    # three segments: segment 0 is not the path's last
    sc = _scene(cr, data, w, h, depth=3, prime=rvs)
    _render(sc, rvs, 1)
    assert not sc.debug_last_build() and not sc.debug_lean_build()
    sc.close()
    # the 32-triangle box: a tree of a few nodes takes the plain per-lane loops, never a one-pass build
    sc = _scene(cr, cornell_data, w, h, prime=rvs)
    _render(sc, rvs, 1)
    assert not sc.debug_launch_info()["one_pass"] and not sc.debug_lean_build()
    sc.close()
    # a tree built on the device never went through the create-time validator: it keeps the checked pushes
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    sc = _scene(cr, cr.SceneData.for_device_build(tessellated_cornell(cornell[0], 8), cornell[1], builder="sah"), w, h, prime=rvs)
    _render(sc, rvs, 1)
    assert sc.debug_launch_info()["one_pass"] and sc.debug_last_build() and not sc.debug_lean_build()
    sc.close()


@pytest.mark.gpu
def test_first_frame_of_a_view_measures_tile_costs_in_the_other_build(cr, scenes, rvs):
    """A frame of several tiles: the one launch that clocks the tiles of a new view is not LEAN (the form has no clock in it), the next
    one is, and the sum of either is the sum with the option off."""
    w, h = 130, 70                                                # 9 x 5 tiles of 16 x 16
    sc = _scene(cr, scenes["lambert"][0], w, h)
    sc.set_option("lean_build", 1)
    sc.render_frames(rvs)
    first = (sc.debug_lean_build(), sc.read_sum())
    sc.reset(); sc.render_frames(rvs)
    second = (sc.debug_lean_build(), sc.read_sum())
    off, _ = _render(sc, rvs, 0)
    print("first launch lean", first[0], "second", second[0])
    assert not first[0] and second[0] and not sc.debug_lean_build()
    assert off.max() > 0
    assert np.array_equal(first[1].view(np.uint32), off.view(np.uint32)) and np.array_equal(second[1].view(np.uint32), off.view(np.uint32))
    sc.close()


@pytest.mark.gpu
def test_lean_sine_and_cosine_have_the_legacy_bits(tmp_path):
    """tools/ubench/pinned_exhaustive.hip: the LEAN and the legacy pinned_sin / pinned_cos on 2^24 floats (every exponent 2^-30 .. 2^30,
    +-0, around +-1e9, +-inf, NaN, the 4,096 floats nearest to each of +-k pi, k = 1 .. 64, and to each of +-(k + 1/2) pi, k = 0 .. 63, where
    the parity of rint(x / pi) flips): zero differing bit patterns."""
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.fail("hipcc not found")
    exe = str(tmp_path / "pinned_exhaustive")
    subprocess.run([hipcc, "-O3", "-ffp-contract=off", "--offload-arch=gfx950", "-I", os.path.join(ROOT, "caitlynrenderer_amd", "csrc"), "-o", exe,
                    os.path.join(ROOT, "tools", "ubench", "pinned_exhaustive.hip")], check=True, capture_output=True, timeout=300)
    out = subprocess.run([exe], check=True, capture_output=True, text=True, timeout=120).stdout
    print(out)
    m = re.search(r"(\d+) inputs .*pinned_sin differs on (\d+), pinned_cos differs on (\d+); sine not zero on (\d+), cosine negative on (\d+)", out)
    assert m, out
    n, ds, dc, nz, neg = (int(x) for x in m.groups())
    assert n == 1 << 24 and ds == 0 and dc == 0, out
    assert nz > n // 2 and neg > n // 8, out              # the inputs did reach the polynomial, and odd multiples of pi
