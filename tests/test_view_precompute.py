"""The one-pass first-segment launch of a one-segment frame runs a build that is the path's last segment at compile time (option
last_build): no bounce sampling, no next-ray queue, no path state in its code.  What is left does the same operations
on the same operands, so every case here is held to the CPU oracle bit for bit — the radiance sum and the ray and visit counters — with
the option on and off, and the launch has to say which build it ran.

Tessellated Cornell box n = 8 (1,922 triangles), 64x48, four samples through one crt_render_frames call: the form the bench's step has."""

import numpy as np
import pytest

from conftest import _Cam

W, H = 64, 48


def _oracle(ob, data, cam, rvs, w=W, h=H, depth=1):
    """(sum of the four frames, their ray and visit counts added up) from the CPU oracle"""
    orc = ob.Oracle(data, w, h, depth, cam)
    ref = np.zeros((h, w, 3), np.float32)
    cnt = np.zeros(4, np.int64)
    for rx, ry in rvs:
        cnt += np.array(orc.render_frame(rx, ry, ref, threads=8)[1][:4], np.int64)
    assert ref.max() > 0.1
    return ref, cnt


def _check(scene, rvs, ref, cnt, last, one_pass=True, label=""):
    """The four frames as one call, first through the timed builds, then through the counting builds in the same launch form: the sum's bits
    both times, the counters the second time, and whether the launch ran the build compiled as a last segment."""
    for counting in (0, 2):
        scene.set_option("count_visits", counting)
        scene.reset()
        scene.render_frames(rvs)
        st = scene.frame_stats()
        out = scene.read_sum()
        print(label, "counting" if counting else "timed", scene.debug_launch_info(), "last build", scene.debug_last_build(),
              "max |d| vs oracle", float(np.abs(out - ref).max()))
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (label, counting)
        assert (st["closest_rays"], st["any_rays"]) == (cnt[0], cnt[1]) and st["stack_overflows"] == 0, (label, counting)
        if counting:
            assert st["nodes_closest"] + st["nodes_any"] == cnt[2] and st["tris_closest"] + st["tris_any"] == cnt[3], label
        if one_pass:
            assert scene.debug_launch_info()["one_pass"] and scene.debug_launch_info()["samples"] == 4, (label, counting)
        assert scene.debug_last_build() == bool(last), (label, counting)
    scene.set_option("count_visits", 0)


@pytest.fixture(scope="module")
def rvs(cr):
    rnd = cr.Rnd()
    return [(rnd.randf2(), rnd.randf2()) for _ in range(4)]


@pytest.fixture(scope="module")
def plain(cr, ob, cornell, tess8, rvs):
    """(scene data, oracle sum, oracle counts) of the Lambert scene at the first pose"""
    return (tess8[1],) + _oracle(ob, tess8[1], cornell[1], rvs)


@pytest.fixture(scope="module")
def disney(cr, ob, cornell, rvs):
    from caitlynrenderer_amd.meshgen import tessellated_cornell, with_disney_materials
    data = cr.SceneData.build(tessellated_cornell(with_disney_materials(cornell[0]), 8), cornell[1])
    return (data,) + _oracle(ob, data, cornell[1], rvs)


def _scene(cr, data, w=W, h=H, depth=1):
    sc = cr.Scene(data, w, h, depth)
    sc.set_option("wide_first", 1)      # a Lambert scene's one-pass build is the 6-wave one, which a frame this small would not pick by itself
    return sc


def _second_pose(cr, cornell):
    c = cornell[1].c
    d = {k: [float(getattr(c, k)[i]) for i in range(3)] for k in ("position", "right", "up", "forward")}
    d["position"] = [d["position"][0] + 0.75, d["position"][1] - 0.5, d["position"][2] + 1.25]
    d["fov"] = float(c.fov)
    return _Cam(cr, d)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["lambert", "disney"])
def test_option_on_and_off(cr, plain, disney, rvs, which):
    """The Lambert scene runs the headline's build <FIRST, INPLACE, BATCH, WIDE, ONE>, the Disney scene the MAT one (its mirror and Disney
    branches have bounce code of their own to leave out), the counting pass of either the STATS one."""
    data, ref, cnt = plain if which == "lambert" else disney
    sc = _scene(cr, data)
    for last in (1, 0, 1):
        sc.set_option("last_build", last)
        _check(sc, rvs, ref, cnt, last, label=f"{which} last_build {last}")
    sc.close()


@pytest.mark.gpu
def test_camera_to_a_second_pose_and_back(cr, ob, cornell, plain, rvs):
    """The LAST build keeps nothing from one view to the next, so nothing here can go stale: the case only holds the build to the oracle
    at a second pose, and checks that a camera update leaves the choice of build alone."""
    data, ref, cnt = plain
    cam2 = _second_pose(cr, cornell)
    ref2, cnt2 = _oracle(ob, data, cam2, rvs)
    assert not np.array_equal(ref2, ref)
    sc = _scene(cr, data)
    for last in (1, 0):
        sc.set_option("last_build", last)
        _check(sc, rvs, ref, cnt, last, label=f"pose 1 last_build {last}")
        sc.update(cam2)
        _check(sc, rvs, ref2, cnt2, last, label=f"pose 2 last_build {last}")
        sc.update(cornell[1])
        _check(sc, rvs, ref, cnt, last, label=f"pose 1 again last_build {last}")
    sc.close()


@pytest.mark.gpu
def test_update_vertices_moves_one_box(cr, ob, cornell, tess8, plain, rvs):
    """The LAST build reads the records as every build does and holds no copy of them: this is the build on a refitted tree, not a guard
    of per-view state.  The oracle walks the trees as the host refits them (the device refit's bytes equal those: test_refit.py), so the
    visit counters are held too."""
    mesh = tess8[0]
    data, ref, cnt = plain
    V = mesh.vertices.copy()
    V[:5 * 81] += np.array([0.5, 0.0, 0.25], np.float32)        # the first five quads of 9 x 9 vertices: the tall box

    def refitted(vertices):
        d = cr.SceneData.build(mesh, cornell[1])
        sb = cr.SBVH.__new__(cr.SBVH)
        sb.flat_nodes, sb.triangles = np.ascontiguousarray(data.bvh, np.float32).copy(), np.ascontiguousarray(data.triangles, np.int32)
        cw = cr.CWBVH()
        cw.nodes, cw.tri_slots = np.ascontiguousarray(data.bvh8, np.uint8).copy(), np.ascontiguousarray(data.bvh8_tri_slots, np.int32)
        d.vertices, d.bvh, d.bvh8 = vertices, sb.refit(vertices).flat_nodes, cw.refit(data.triangles, vertices).nodes
        return _oracle(ob, d, cornell[1], rvs)
    ref0, cnt0 = refitted(mesh.vertices)            # moved back: the same picture as created, through refitted boxes
    ref1, cnt1 = refitted(V)
    assert np.array_equal(ref0, ref) and not np.array_equal(ref1, ref)
    sc = _scene(cr, data)
    _check(sc, rvs, ref, cnt, 1, label="as created")
    for last in (1, 0):
        sc.set_option("last_build", last)
        sc.update_vertices(V)
        _check(sc, rvs, ref1, cnt1, last, label=f"box moved last_build {last}")
        sc.update_vertices(mesh.vertices)
        _check(sc, rvs, ref0, cnt0, last, label=f"moved back last_build {last}")
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("split", ["streams", "devices"])
def test_two_streams_and_two_virtual_devices(cr, cornell, plain, rvs, split):
    """The option reaches every shard's launches (set before and after the split)."""
    data, ref, cnt = plain
    sc = _scene(cr, data)
    sc.set_option("last_build", 0)
    if split == "streams":
        sc.set_option("streams", 2)
    else:
        sc.set_devices([0, 0])
    sc.update(cornell[1])
    assert sc.debug_launch_info()["shards"] == 2
    _check(sc, rvs, ref, cnt, 0, label=f"{split} last_build 0 from before the split")
    for last in (1, 0):
        sc.set_option("last_build", last)
        _check(sc, rvs, ref, cnt, last, label=f"{split} last_build {last}")
    sc.close()


@pytest.mark.gpu
def test_two_segments_keep_the_unspecialised_first_segment(cr, ob, cornell, plain, rvs):
    """At depth 2 segment 0 is not the last one: whatever the option says its launch is not the LAST build, it samples the bounce and
    queues the next ray, and segment 1 is a queue-fed launch the option does not reach — sums and counters of both as the oracle has them."""
    data = plain[0]
    ref, cnt = _oracle(ob, data, cornell[1], rvs, depth=2)
    sc = _scene(cr, data, depth=2)
    for last in (1, 0):
        sc.set_option("last_build", last)
        _check(sc, rvs, ref, cnt, 0, one_pass=False, label=f"depth 2 last_build {last}")
    sc.close()


@pytest.mark.gpu
def test_frame_that_is_no_multiple_of_the_tile(cr, ob, cornell, plain, rvs):
    """70x50 with 16-pixel tiles: the tiles of the right and the lower edge reach beyond the frame, so some lanes of the LAST build's waves
    own no pixel (the build computes its pixel quotients as every build does: there are no per-view tables to index past)."""
    data = plain[0]
    ref, cnt = _oracle(ob, data, cornell[1], rvs, 70, 50)
    sc = _scene(cr, data, 70, 50)
    for last in (1, 0):
        sc.set_option("last_build", last)
        _check(sc, rvs, ref, cnt, last, label=f"70x50 last_build {last}")
    sc.close()
