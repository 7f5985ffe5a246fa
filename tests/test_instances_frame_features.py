"""Per-instance material offsets and visibility masks in the frames of an instanced scene (include/crt.h crt_scene_create_instanced;
DESIGN.md §17).  Every comparison is bit for bit: the CPU oracle walks masked (ob.trace_instances with ob.INSTANCE_MASK, ray masks in
the rays' pad words) and renders the flat scenes the instanced ones must equal.

CPU: the layouts, the null-handle refusals, and the premises that let the GPU checks fail (1, 2a - 2c of the change's issue).
GPU: M1 - M3 (offsets against the flat oracle, under general transforms, refusals), V1 - V6 (the option on with nothing hidden, parts
hidden from every class, from shadow rays only, from the camera only, each class with its own mask, shards and interleaving) and the
option refusals.  The helpers are those of tests/test_instances_frames.py and tests/test_instances_oracle.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from test_instances_frames import (RVS, THREADS, close, emissive_meshes, f32_dot, flat_variants, look_at, oracle_frames, primary_oracle,
                                   shading_of, split_mesh)
from test_instances_oracle import IDENTITY, host_blas, host_scene, orc, placed_instances

f32 = np.float32
W3, H3 = 231, 130
SIZES = ((67, 45), (231, 130))
DEPTHS = (1, 3, 4)


# ---------------------------------------------------------------- helpers ----

def with_triangles(cr, mesh, triangles):
    return cr.Mesh(mesh.vertices, mesh.normals, mesh.texcoords, triangles, mesh.materials, mesh.lights, mesh.vertex_min)


def lowered(cr, meshes):
    """each mesh with v[3] lowered by its minimum, and the minima: what the instances give back as material offsets"""
    lo = np.array([int(m.triangles[:, 3].min()) for m in meshes])
    out = []
    for m, k in zip(meshes, lo):
        t = m.triangles.copy()
        t[:, 3] -= k
        out.append(with_triangles(cr, m, t))
    return out, lo


def identity_scene(cr, meshes, mesh, cam, W, H, depth, builder="sah", masks=None, offsets=None, options=(), shard=None, **kw):
    n = len(meshes)
    inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY] * n, np.arange(n), masks, offsets), builder=builder, **kw)
    sc = inst.frame_scene(shading_of(meshes), mesh.materials, mesh.lights, W, H, depth, textures=mesh.albedo_textures)
    sc.update(cam)
    if shard:
        sc.set_shard(shard[0], shard[1], 16)
    for name, value in options:
        sc.set_option(name, value)
    return inst, sc


def frames(sc, n_frames=3, sync=True):
    for rx, ry in RVS[:n_frames]:
        sc.render_frame(rx, ry, sync=sync)


def assert_same_bits(got, want, what=()):
    bad = np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(-1))
    assert bad[0].size == 0, (what, bad[0].size, got[bad][:3], want[bad][:3])


def masks_on(primary=255, bounce=255, shadow=255):
    return (("instance_masks", 1), ("mask_primary", primary), ("mask_bounce", bounce), ("mask_shadow", shadow))


_FLAT = {}


def flat_frames(cr, ob, key, mesh, cam, W, H, depth, n_frames=3):
    """(sum, counters of the last frame) of the flat oracle on `mesh`, once per key"""
    key = (key, W, H, depth, n_frames)
    if key not in _FLAT:
        o = ob.Oracle(cr.SceneData.build(mesh, cam), W, H, depth)
        ref = np.zeros((H, W, 3), f32)
        cnt = None
        for rx, ry in RVS[:n_frames]:
            _, cnt = o.render_frame(rx, ry, ref, accel=ob.BVH8, tie=ob.TIE_LOWEST_ID, threads=THREADS)
        _FLAT[key] = (ref, cnt)
    return _FLAT[key]


def without_parts(cr, mesh, parts, hidden):
    """the flat mesh without the triangles of the hidden parts of its `parts`-way split, the rest in their order (same lights)"""
    n = mesh.triangles.shape[0]
    cuts = [n * k // parts for k in range(parts + 1)]
    keep = np.concatenate([np.arange(cuts[p], cuts[p + 1]) for p in range(parts) if p not in hidden])
    m = with_triangles(cr, mesh, mesh.triangles[keep])
    m.albedo_textures = mesh.albedo_textures
    return m


def handle_arrays(inst):
    """what the walk reads, through debug reads 2 - 5 (never 6: the child masks are the oracle's own OR over the records)"""
    info = inst.info()
    return dict(tlas=inst.tlas_nodes(), inst=inst.instance_records(), blas=inst.blas_nodes(), recs=inst.blas_records(),
                region=info["tlas_bytes"] // 80, stack=info["stack_entries"])


def walk(ob, a, rays, mode, mask=None):
    """the CPU two-level walk of `rays`; mask: the class's ray mask, written over the rays' pad words (payloads, in a queue)"""
    r = rays.copy()
    if mask is not None:
        r["pad"] = mask
        mode |= ob.INSTANCE_MASK
    hits, ids, st, _, refused = ob.trace_instances(a["tlas"], a["inst"], a["blas"], a["recs"], r, a["region"], a["stack"], mode, threads=THREADS)
    assert refused.sum() == 0
    return hits, ids, st


def counts(st):
    return int(st["nodes"].astype(np.int64).sum()), int(st["tris"].astype(np.int64).sum())


def emission_frames(cr, ob, inst, sc, meshes, table, mesh_of, offs, cam, W, H, ray_mask=None, k_frames=3):
    """depth-1 frames of an all-emissive scene: the sum is the float32 accumulation of emission[v[3] + offset(instance)] over the oracle's
    (masked) primary hits, the closest-hit visit totals are the oracle's sums"""
    po = primary_oracle(ob, cam, W, H)
    a = handle_arrays(inst)
    want = np.zeros((H * W, 3), f32)
    sc.reset()
    sc.set_option("count_visits", 1)
    seen = set()
    for rx, ry in RVS[:k_frames]:
        sc.render_frame(rx, ry)
        rays = po.primary_rays(rx, ry, jitter=True)
        hits, ids, st = walk(ob, a, rays, ob.CLOSEST, ray_mask)
        hit = ids >= 0
        i = np.maximum(ids, 0)
        mat = np.zeros(H * W, np.int64)
        for m in range(len(meshes)):
            sel = hit & (mesh_of[i] == m)
            mat[sel] = meshes[m].triangles[hits["tri"][sel], 3]
        mat = np.where(hit, mat + offs[i], 0)
        assert mat.max() < table.shape[0]
        e = np.where(hit[:, None], table[mat, 4:7], f32(0)).astype(f32)
        want = (e + want).astype(f32)
        fs = sc.frame_stats()
        assert (fs["nodes_closest"], fs["tris_closest"]) == counts(st), (fs["nodes_closest"], fs["tris_closest"], counts(st))
        assert fs["closest_rays"] == W * H and fs["stack_overflows"] == 0
        seen |= set(zip(mesh_of[i[hit]].tolist(), offs[i[hit]].tolist()))
    assert_same_bits(sc.read_sum().reshape(-1, 3), want)
    assert hit.mean() > 0.2
    sc.set_option("count_visits", 0)
    return seen, ids


def emissive_table(mats, extra):
    """emissive_meshes' 6 emissive materials + `extra` more, every colour distinct"""
    rng = np.random.default_rng(78)
    t = np.concatenate([mats, np.repeat(mats[:1], extra, 0)])
    t[6:, 4:7] = rng.uniform(0.1, 4.0, (extra, 3))
    assert np.unique(t[:, 4:7], axis=0).shape[0] == t.shape[0]
    return t.astype(f32)


def random_offsets(rng, meshes, mesh_of, n_materials):
    hi = np.array([int(m.triangles[:, 3].max()) for m in meshes])
    return rng.integers(0, n_materials - hi[mesh_of]).astype(np.uint32)           # hi + offset <= n_materials - 1


# ---------------------------------------------------------------- CPU 1: layouts and null handles ----

def test_material_offset_is_the_word_at_byte_56(cr):
    from caitlynrenderer_amd import _lib
    rng = np.random.default_rng(5)
    M, mesh_of = placed_instances(rng, 9, 3)
    masks = rng.integers(0, 256, 9)
    offs = np.array([0, 1, 7, 0x7fffffff, 0x80000000, 0xffffffff, 3, 0, 12], np.uint32)
    plain, got = cr.instances_array(M, mesh_of, masks), cr.instances_array(M, mesh_of, masks, material_offsets=offs)
    assert got.dtype.itemsize == 64 and got.tobytes() != plain.tobytes()
    raw, base = np.frombuffer(got.tobytes(), np.uint8).reshape(9, 64), np.frombuffer(plain.tobytes(), np.uint8).reshape(9, 64)
    assert np.array_equal(raw[:, 56:60].copy().view(np.uint32)[:, 0], offs)
    assert np.array_equal(raw[:, :56], base[:, :56]) and not raw[:, 60:].any() and not base[:, 56:].any()
    # the default is the array of before: matrices, mesh and mask words, zeros behind them
    old = np.zeros(9, np.dtype([("object_to_world", "<f4", 12), ("mesh", "<u4"), ("mask", "<u4"), ("reserved", "<u4", 2)]))
    old["object_to_world"], old["mesh"], old["mask"] = M.reshape(9, 12), mesh_of, masks
    assert plain.tobytes() == old.tobytes()
    assert cr.instances_array(M, mesh_of).tobytes() == cr.instances_array(M, mesh_of, np.zeros(9), np.zeros(9)).tobytes()
    # the binding's struct: the same word under both names
    rec = _lib.crt_instance()
    rec.material_offset = 0xdeadbeef
    assert C.sizeof(_lib.crt_instance) == 64 and _lib.crt_instance.material_offset.offset == 56 and rec.reserved[0] == 0xdeadbeef
    # the C struct of the header, read as tests/test_abi.py reads it: comments stripped
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "crt.h")).read(), flags=re.S)
    body = re.search(r"typedef\s+struct\s+crt_instance\s*\{(.*?)\}\s*crt_instance\s*;", src, flags=re.S).group(1)
    at, offset = 0, {}
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(float|uint32_t)\s+(\w+)(?:\[(\d+)\])?", decl)
        assert m, decl
        offset[m.group(2)] = at
        at += 4 * int(m.group(3) or 1)
    assert at == 64 and offset["material_offset"] == 56 and offset["mask"] == 52 and offset["mesh"] == 48


def test_null_handle_calls_of_the_mask_options_fail_loudly(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    for name in (b"instance_masks", b"mask_primary", b"mask_bounce", b"mask_shadow"):
        assert L.crt_set_option(None, name, 1) == _lib.CRT_ERR_INVALID
        assert len(L.crt_last_error()) > 10


# ---------------------------------------------------------------- CPU 2: premises ----

@pytest.mark.parametrize("name", ["cornell", "textured", "tess8_mat"])
def test_premise_offsets_give_the_flat_materials_back(cr, cornell, textured, name):
    """2a: v[3] lowered by the mesh's minimum + the instance's offset is the flat material of every triangle, and M1 runs non-zero offsets"""
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    meshes, first = split_mesh(cr, mesh, parts)
    low, lo = lowered(cr, meshes)
    for k, m in enumerate(low):
        assert m.triangles[:, 3].min() == 0
        assert np.array_equal(m.triangles[:, 3] + lo[k], mesh.triangles[first[k]:first[k] + m.triangles.shape[0], 3])
    assert (lo != 0).sum() >= 2, lo
    if name == "cornell":
        assert lo.tolist() == [3, 3, 0, 1]


def on_part(cr, ob, mesh, cam, a, b):
    """per frame of RVS[:3] at W3 x H3: which pixels' primary hit is a triangle of [a, b)"""
    o = ob.Oracle(cr.SceneData.build(mesh, cam), W3, H3, 1)
    out = []
    for rx, ry in RVS[:3]:
        hits = o.trace(o.primary_rays(rx, ry, jitter=True), ob.BVH8, ob.CLOSEST, ob.TIE_LOWEST_ID, threads=THREADS)
        out.append((hits["tri"] >= a) & (hits["tri"] < b))
    return np.array(out).reshape(3, H3, W3)


def test_premise_the_shadow_of_part_1_is_in_the_picture(cr, ob, cornell):
    """2b: V3 can fail — X (triangles [8, 16) of the Cornell box) is seen, and pixels never on X change when X's triangles go"""
    mesh, cam = cornell
    on = on_part(cr, ob, mesh, cam, 8, 16)
    share = on.reshape(3, -1).mean(1)
    assert ((share >= 0.02) & (share <= 0.25)).any() and on.any(0).mean() <= 0.25, share
    with_x, _ = flat_frames(cr, ob, "cornell", mesh, cam, W3, H3, 1)
    no_x, _ = flat_frames(cr, ob, "cornell-1", without_parts(cr, mesh, 4, {1}), cam, W3, H3, 1)
    differ = (with_x.view(np.uint32) != no_x.view(np.uint32)).any(-1)
    print("on X: %.1f %%; pixels never on X that differ: %d; on X that differ: %d of %d"
          % (100 * on.any(0).mean(), (differ & ~on.any(0)).sum(), (differ & on.any(0)).sum(), on.any(0).sum()))
    assert (differ & ~on.any(0)).sum() >= 50


V5_MASKS = np.array([1, 2, 4, 3, 5, 6, 7], np.uint32)


def v5_scene(cr, cornell, tess8):
    meshes, mats, light = emissive_meshes(cr, cornell, tess8, lambert=True)
    rng = np.random.default_rng(403)
    M, mesh_of = placed_instances(rng, 120, 3, spread=8.0)
    mesh_of[:3] = (0, 1, 2)
    masks = V5_MASKS[rng.integers(0, V5_MASKS.shape[0], 120)]
    return meshes, mats, light, M, mesh_of, masks


def test_premise_masks_change_the_visit_counts_of_every_class(cr, ob, cornell, tess8):
    """2c: V5's counters can tell a masked walk from an unmasked one — on host-assembled arrays the oracle's summed node counts differ
    between the two for primary rays under mask 1, bounce-like rays under mask 2 and shadow-like rays under mask 4"""
    meshes, mats, light, M, mesh_of, masks = v5_scene(cr, cornell, tess8)
    s = host_scene(cr, [host_blas(cr, m) for m in meshes], M, mesh_of, masks)
    W, H = 160, 96
    rays = primary_oracle(ob, look_at(cr, (2.0, 3.0, 28.0), (0.0, 0.0, 0.0)), W, H).primary_rays(*RVS[0], jitter=True)
    rays["pad"] = 1
    hits, ids, st, _, _ = orc(ob, s, rays, ob.CLOSEST, masked=True)
    hit = ids >= 0
    assert hit.sum() > 1000
    point = (rays["o"][hit] + rays["d"][hit] * (hits["t"][hit] * f32(0.999))[:, None]).astype(f32)
    rng = np.random.default_rng(404)
    d = rng.normal(size=point.shape)
    bounce = np.zeros(point.shape[0], cr.RAY_DT)
    bounce["o"], bounce["d"], bounce["tmax"], bounce["pad"] = point, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(f32), f32(1e9), 2
    centre = (light[0, 0:3] + (light[0, 3:6] + light[0, 6:9]) / 3).astype(np.float64)
    to = centre[None] - point
    shadow = bounce.copy()
    shadow["d"], shadow["tmax"], shadow["pad"] = (to / np.linalg.norm(to, axis=1, keepdims=True)).astype(f32), (np.linalg.norm(to, axis=1) - 1e-4).astype(f32), 4
    for r, mode in ((rays, ob.CLOSEST), (bounce, ob.CLOSEST), (shadow, ob.ANY)):
        masked, plain = orc(ob, s, r, mode, masked=True)[2], orc(ob, s, r, mode)[2]
        assert counts(masked)[0] != counts(plain)[0], (mode, counts(masked), counts(plain))


# ---------------------------------------------------------------- M1, V1: offsets and the option against the flat oracle ----

@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "textured", "tess8_mat"])
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
def test_m1_offsets_render_the_flat_oracles_frames(cr, ob, cornell, textured, name, builder):
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    low, lo = lowered(cr, split_mesh(cr, mesh, parts)[0])
    for W, H in SIZES:
        for depth in DEPTHS:
            ref, cnt = oracle_frames(cr, ob, name, mesh, cam, W, H, depth)
            inst, sc = identity_scene(cr, low, mesh, cam, W, H, depth, builder, offsets=lo)
            frames(sc)
            assert_same_bits(sc.read_sum(), ref, (name, builder, W, H, depth))
            st = sc.frame_stats()
            assert (st["closest_rays"], st["any_rays"]) == (cnt[0], cnt[1]) and st["stack_overflows"] == 0
            close(inst, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "textured", "tess8_mat"])
def test_v1_the_option_on_with_nothing_hidden(cr, ob, cornell, textured, name):
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    low, lo = lowered(cr, split_mesh(cr, mesh, parts)[0])
    for masks in (np.full(parts, 0xff), 1 << (np.arange(parts) % 8)):
        for W, H in SIZES:
            for depth in DEPTHS:
                ref, cnt = oracle_frames(cr, ob, name, mesh, cam, W, H, depth)
                inst, sc = identity_scene(cr, low, mesh, cam, W, H, depth, masks=masks, offsets=lo, options=masks_on())
                frames(sc)
                assert_same_bits(sc.read_sum(), ref, (name, masks[:2], W, H, depth))
                st = sc.frame_stats()
                assert (st["closest_rays"], st["any_rays"]) == (cnt[0], cnt[1]) and st["stack_overflows"] == 0
                close(inst, sc)


# ---------------------------------------------------------------- M2, V4: general transforms, one BLAS, many looks ----

def m2_scene(cr, cornell, tess8, seed, n, capacity=300):
    meshes, mats, light = emissive_meshes(cr, cornell, tess8)
    table = emissive_table(mats, 5)
    rng = np.random.default_rng(seed)
    M, mesh_of = placed_instances(rng, n, 3, spread=9.0)
    mesh_of[:3] = (0, 1, 2)
    offs = random_offsets(rng, meshes, mesh_of, table.shape[0])
    return meshes, table, light, rng, M, mesh_of, offs


@pytest.mark.gpu
def test_m2_offsets_under_general_transforms(cr, ob, cornell, tess8):
    meshes, table, light, rng, M, mesh_of, offs = m2_scene(cr, cornell, tess8, 411, 120)
    inst = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of, material_offsets=offs), capacity=300)
    W, H = 160, 96
    cam = look_at(cr, (2.0, 3.0, 30.0), (0.0, 0.0, 0.0))
    sc = inst.frame_scene(shading_of(meshes), table, light, W, H, 1)
    sc.update(cam)
    seen, ids0 = emission_frames(cr, ob, inst, sc, meshes, table, mesh_of, offs, cam, W, H)
    # one BLAS, several looks: the hit instances of the box and of its tessellation carry >= 3 different offsets each.  (The third mesh, a
    # 2 x 2 quad seen from 30 units away, covers a few pixels only: the oracle finds one of its 39 instances in these frames.)
    looks = [len({o for k, o in seen if k == m}) for m in range(3)]
    assert looks[0] >= 3 and looks[1] >= 3, (looks, seen)
    # a refit that changes only offsets: the same hits, other colours
    offs2 = random_offsets(rng, meshes, mesh_of, table.shape[0])
    assert (offs2 != offs).mean() > 0.5
    inst.refit(cr.instances_array(M, mesh_of, material_offsets=offs2))
    _, ids1 = emission_frames(cr, ob, inst, sc, meshes, table, mesh_of, offs2, cam, W, H)
    assert np.array_equal(ids0, ids1)
    # and a set to another count
    M3, mesh_of3 = placed_instances(rng, 260, 3, spread=9.0)
    mesh_of3[:3] = (0, 1, 2)
    offs3 = random_offsets(rng, meshes, mesh_of3, table.shape[0])
    inst.set(cr.instances_array(M3, mesh_of3, material_offsets=offs3))
    emission_frames(cr, ob, inst, sc, meshes, table, mesh_of3, offs3, cam, W, H)
    close(inst, sc)


@pytest.mark.gpu
def test_v4_hidden_from_the_camera_only(cr, ob, cornell, tess8):
    meshes, table, light, rng, M, mesh_of, offs = m2_scene(cr, cornell, tess8, 412, 120)
    masks = np.where(np.arange(120) % 3 == 0, 2, 1)       # a third of the instances: not for mask_primary 1
    inst = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of, masks, offs))
    W, H = 160, 96
    cam = look_at(cr, (2.0, 3.0, 30.0), (0.0, 0.0, 0.0))
    sc = inst.frame_scene(shading_of(meshes), table, light, W, H, 1)
    sc.update(cam)
    _, plain = emission_frames(cr, ob, inst, sc, meshes, table, mesh_of, offs, cam, W, H)
    for name, value in masks_on(primary=1):
        sc.set_option(name, value)
    _, ids = emission_frames(cr, ob, inst, sc, meshes, table, mesh_of, offs, cam, W, H, ray_mask=1)
    assert (ids[ids >= 0] % 3 != 0).all() and (plain[plain >= 0] % 3 == 0).mean() > 0.1        # the hidden third was in the picture
    close(inst, sc)


# ---------------------------------------------------------------- M3: refusals ----

@pytest.mark.gpu
def test_m3_offsets_are_held_to_the_bound_scenes_material_table(cr, ob, cornell):
    import torch
    from caitlynrenderer_amd import _lib
    mesh, cam = cornell
    meshes, _ = split_mesh(cr, mesh, 4)                   # no texcoords at all: no mesh may land on a textured material
    nm = mesh.materials.shape[0]
    lo = np.array([int(m.triangles[:, 3].min()) for m in meshes])
    hi = np.array([int(m.triangles[:, 3].max()) for m in meshes])
    textured_entry = mesh.materials[:1].copy()
    textured_entry[0, 12] = 0
    table = np.concatenate([mesh.materials, textured_entry, mesh.materials]).astype(f32)        # material nm is textured
    n_mat = table.shape[0]
    tex = np.full((1, 4, 4, 3), 200, np.uint8)
    W, H = 67, 45

    def arr(offsets):
        return cr.instances_array([IDENTITY] * 4, np.arange(4), material_offsets=offsets)

    def scene(inst):
        sc = inst.frame_scene(shading_of(meshes), table, mesh.lights, W, H, 3, textures=tex)
        sc.update(cam)
        return sc

    zero = np.zeros(4, np.uint32)
    past_end, last, sign = zero.copy(), zero.copy(), zero.copy()
    past_end[2], last[2], sign[1] = n_mat - hi[2], n_mat - 1 - hi[2], 0x80000000
    onto, past = zero.copy(), zero.copy()
    onto[3], past[3] = nm - lo[3], nm + 1 - lo[3]         # mesh 3's least material lands on the textured one / just past it
    assert lo[3] + past[3] > nm and hi[3] + past[3] < n_mat and lo[2] + last[2] > nm
    refused = (past_end, sign, onto)
    # create: the rule on the handle's LIVE instances; a handle without a bound scene stores any offset
    for bad in refused:
        inst = cr.InstancedScene(meshes, arr(bad), capacity=8)
        with pytest.raises(cr.CrtError) as e:
            scene(inst)
        assert e.value.code == _lib.CRT_ERR_INVALID and "material_offset" in str(e.value), str(e.value)
        inst.close()                                      # nothing was bound
    inst = cr.InstancedScene(meshes, arr(last), capacity=8)
    sc = scene(inst)
    frames(sc, 2)
    before = sc.read_sum()
    assert before.any()

    def unchanged():
        sc.reset()
        frames(sc, 2)
        assert_same_bits(sc.read_sum(), before)

    for bad in refused:
        dev = torch.from_numpy(np.frombuffer(arr(bad).tobytes(), np.uint8).copy()).cuda()
        for call in (lambda: inst.set(arr(bad)), lambda: inst.refit(arr(bad)), lambda: inst.set_device(dev.data_ptr(), 4),
                     lambda: inst.refit_device(dev.data_ptr(), 4)):
            with pytest.raises(cr.CrtError) as e:
                call()
            assert e.value.code == _lib.CRT_ERR_INVALID and "material_offset" in str(e.value), str(e.value)
            unchanged()
    with pytest.raises(cr.CrtError) as e:
        inst.set(arr(onto))
    assert "instance 3" in str(e.value) and "textured" in str(e.value), str(e.value)
    # accepted: the last material, past the textured one, and a count change carrying offsets
    for good in (past, last, zero):
        inst.refit(arr(good))
        inst.set(arr(good))
    inst.set(arr(last))
    unchanged()
    sc.close()
    inst.set(arr(past_end))                               # unbound: accepted again
    inst.close()


@pytest.mark.gpu
def test_m3_ray_queries_never_read_the_offset(cr, ob, cornell, tess8):
    meshes, table, light, rng, M, mesh_of, offs = m2_scene(cr, cornell, tess8, 413, 90)
    offs[::4] = rng.integers(1 << 20, 1 << 32, offs[::4].shape[0], dtype=np.uint64).astype(np.uint32)       # unbound: anything goes
    masks = rng.integers(0, 256, 90)
    a = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of, masks, offs), updatable=True)
    b = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of, masks), updatable=True)
    rays = primary_oracle(ob, look_at(cr, (2.0, 3.0, 30.0), (0.0, 0.0, 0.0)), 160, 96).primary_rays(*RVS[0], jitter=True)
    for mode in (cr.CRT_TRACE_CLOSEST, cr.CRT_TRACE_ANY):
        for ray_mask in (None, 5):
            ra, rb = a.trace(rays, mode, stats=True, ray_mask=ray_mask), b.trace(rays, mode, stats=True, ray_mask=ray_mask)
            for x, y in zip(ra, rb):
                assert x.tobytes() == y.tobytes(), (mode, ray_mask)
    for which, (dtype, width) in enumerate([(f32, 12), (f32, 6), (np.uint8, 80), (f32, 16), (np.uint8, 80), (f32, 12), (np.uint8, 8)]):
        assert a._read(which, dtype, width).tobytes() == b._read(which, dtype, width).tobytes(), which
    a.close()
    b.close()


# ---------------------------------------------------------------- V2, V6: parts hidden from every class ----

V2_CASES = {"cornell": {1}, "tess8_mat": {1, 4, 5}}


def v2_masks(parts, hidden, case):
    """case 0: the hidden parts have mask 0 under class masks 0xff; case 1: mask 2 under class masks 1 (the others 1 or 3)"""
    k = np.arange(parts)
    if case == 0:
        return np.where(np.isin(k, list(hidden)), 0, 0xff), masks_on()
    return np.where(np.isin(k, list(hidden)), 2, 1 + 2 * (k & 1)), masks_on(1, 1, 1)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["cornell", "tess8_mat"])
@pytest.mark.parametrize("case", [0, 1])
def test_v2_hidden_parts_are_in_no_picture_and_come_back_by_a_refit(cr, ob, cornell, textured, name, case):
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    hidden = V2_CASES[name]
    meshes, _ = split_mesh(cr, mesh, parts)
    rest = without_parts(cr, mesh, parts, hidden)
    masks, options = v2_masks(parts, hidden, case)
    W, H = W3, H3
    for depth in DEPTHS:
        ref, cnt = flat_frames(cr, ob, name + "-hidden", rest, cam, W, H, depth)
        full, _ = oracle_frames(cr, ob, name, mesh, cam, W, H, depth)
        assert (ref.view(np.uint32) != full.view(np.uint32)).any(-1).mean() > 0.02           # the hidden parts matter
        inst, sc = identity_scene(cr, meshes, mesh, cam, W, H, depth, masks=masks, options=options)
        frames(sc)
        assert_same_bits(sc.read_sum(), ref, (name, case, depth))
        st = sc.frame_stats()
        assert (st["closest_rays"], st["any_rays"]) == (cnt[0], cnt[1]) and st["stack_overflows"] == 0
        # shown again by a refit: no masked trace and no debug read between the refit and the frames (the stale-child-mask path)
        inst.refit(cr.instances_array([IDENTITY] * parts, np.arange(parts), np.full(parts, 0xff if case == 0 else 1)))
        sc.reset()
        frames(sc)
        assert_same_bits(sc.read_sum(), full, (name, case, depth, "shown"))
        # and hidden again the same way, the frames queued without a wait between them
        inst.refit(cr.instances_array([IDENTITY] * parts, np.arange(parts), masks))
        sc.reset()
        frames(sc, sync=False)
        assert_same_bits(sc.read_sum(), ref, (name, case, depth, "hidden again"))
        close(inst, sc)


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
def test_v6_two_shards_of_a_masked_frame_add_up(cr, ob, cornell, textured, depth):
    from caitlynrenderer_amd import tiles
    name = "tess8_mat"
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    meshes, _ = split_mesh(cr, mesh, parts)
    masks, options = v2_masks(parts, V2_CASES[name], 0)
    ref, _ = flat_frames(cr, ob, name + "-hidden", without_parts(cr, mesh, parts, V2_CASES[name]), cam, W3, H3, depth)
    frame = np.zeros((H3, W3, 3), f32)
    for rank in (0, 1):
        inst, sc = identity_scene(cr, meshes, mesh, cam, W3, H3, depth, masks=masks, options=options, shard=(rank, 2))
        frames(sc)
        part = np.zeros((H3, W3, 3), f32)
        tiles.untile_into(part, sc.read_packed(), tiles.shard_tiles_of_library(W3, H3, 16, rank, 2), 16)
        assert np.array_equal(part.view(np.uint32), sc.read_sum().view(np.uint32))
        frame += part
        close(inst, sc)
    assert_same_bits(frame, ref)


@pytest.mark.gpu
def test_v6_a_masked_trace_between_two_masked_frames(cr, ob, cornell, textured):
    """after a refit the child masks are stale; a frame, a masked crt_instances_trace_device on the handle's stream and two more frames
    are queued with no wait between them: whoever renews the masks, the trace and the frames are exact"""
    import torch
    name, depth = "tess8_mat", 3
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    meshes, _ = split_mesh(cr, mesh, parts)
    masks, options = v2_masks(parts, V2_CASES[name], 1)
    ref, _ = flat_frames(cr, ob, name + "-hidden", without_parts(cr, mesh, parts, V2_CASES[name]), cam, W3, H3, depth)
    inst, sc = identity_scene(cr, meshes, mesh, cam, W3, H3, depth, masks=np.full(parts, 1), options=options)
    rays = ob.Oracle(cr.SceneData.build(mesh, cam), W3, H3, 1).primary_rays(*RVS[0], jitter=True)
    rays["pad"] = np.arange(rays.shape[0]) % 3 + 1        # ray masks 1, 2, 3
    d_rays = torch.from_numpy(np.frombuffer(rays.tobytes(), np.uint8).copy()).cuda()
    d_hits = torch.empty(rays.shape[0] * 16, dtype=torch.uint8, device="cuda")
    d_ids = torch.empty(rays.shape[0], dtype=torch.int32, device="cuda")
    for trace_first in (False, True):
        inst.refit(cr.instances_array([IDENTITY] * parts, np.arange(parts), np.full(parts, 1)))
        frames(sc, 1)                                      # everything visible: masks fresh for THIS state
        inst.refit(cr.instances_array([IDENTITY] * parts, np.arange(parts), masks))            # stale again
        sc.reset()
        if trace_first:
            inst.trace_device(d_rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), d_ids.data_ptr(), cr.CRT_TRACE_CLOSEST | cr.CRT_TRACE_INSTANCE_MASK, sync=False)
        sc.render_frame(*RVS[0], sync=False)
        if not trace_first:
            inst.trace_device(d_rays.data_ptr(), rays.shape[0], d_hits.data_ptr(), d_ids.data_ptr(), cr.CRT_TRACE_CLOSEST | cr.CRT_TRACE_INSTANCE_MASK, sync=False)
        sc.render_frame(*RVS[1], sync=False)
        sc.render_frame(*RVS[2], sync=False)
        assert_same_bits(sc.read_sum(), ref, trace_first)
        inst.info()                                        # waits for the handle's stream
        torch.cuda.synchronize()
        hits, ids, _ = walk(ob, handle_arrays(inst), rays, ob.CLOSEST | ob.INSTANCE_MASK)
        assert d_hits.cpu().numpy().tobytes() == hits.tobytes() and np.array_equal(d_ids.cpu().numpy(), ids)
        assert (ids >= 0).mean() > 0.2 and not np.isin(ids[(rays["pad"] == 1) & (ids >= 0)], list(V2_CASES[name])).any()
    close(inst, sc)


# ---------------------------------------------------------------- V3: hidden from shadow rays only ----

@pytest.mark.gpu
def test_v3_a_part_hidden_from_shadow_rays_casts_no_shadow_and_is_still_seen(cr, ob, cornell):
    mesh, cam = cornell
    meshes, _ = split_mesh(cr, mesh, 4)
    masks = np.array([3, 1, 3, 3])                        # X = part 1: met by the path rays' mask 1, not by the shadow rays' 2
    inst, sc = identity_scene(cr, meshes, mesh, cam, W3, H3, 1, masks=masks, options=masks_on(1, 1, 2))
    frames(sc)
    got = sc.read_sum()
    close(inst, sc)
    no_x, _ = flat_frames(cr, ob, "cornell-1", without_parts(cr, mesh, 4, {1}), cam, W3, H3, 1)
    on = on_part(cr, ob, mesh, cam, 8, 16).any(0)
    assert on.mean() <= 0.25
    differ = (got.view(np.uint32) != no_x.view(np.uint32)).any(-1)
    assert not (differ & ~on).any(), ((differ & ~on).sum(), np.argwhere(differ & ~on)[:4])      # X's shadow is gone, bit for bit
    assert (differ & on).sum() * 4 >= on.sum(), ((differ & on).sum(), on.sum())                  # X itself is still seen


# ---------------------------------------------------------------- V5: every class walks with its own mask ----

def world_hit_points(meshes, mesh_of, inst, rays, hits, ids):
    """contract items 3 - 4 of include/crt.h in numpy float32 (the restatement of tests/test_instances_frames.py's check 5):
    -> (indices of the rays that hit, their hit points (o + d t) + n 0.0002f on the world ray)"""
    rec = inst.instance_records()
    ident = np.zeros(rec.shape[0], bool)
    ident[rec[:, 13].view(np.uint32)] = rec[:, 14].view(np.uint32) != 0
    Wm = inst.world_to_object().reshape(-1, 3, 4)
    hit = np.nonzero(ids >= 0)[0]
    n_obj = np.zeros((hit.size, 3), f32)
    for k, p in enumerate(hit):
        m = meshes[mesh_of[ids[p]]]
        t = m.triangles[hits["tri"][p]]
        if t[7] == 0:
            n_obj[k] = t[4:7].astype(f32)
        else:
            bu, bv = hits["u"][p], hits["v"][p]
            w = f32(f32(f32(1.0) - bu) - bv)
            na, nb, nc = m.normals[t[4]], m.normals[t[5]], m.normals[t[6]]
            n_obj[k] = (((na * w).astype(f32) + (nb * bu).astype(f32)).astype(f32) + (nc * bv).astype(f32)).astype(f32)
    Wh = Wm[ids[hit]]
    with np.errstate(all="ignore"):
        mm = np.stack([(((Wh[:, 0, c] * n_obj[:, 0]).astype(f32) + (Wh[:, 1, c] * n_obj[:, 1]).astype(f32)).astype(f32) + (Wh[:, 2, c] * n_obj[:, 2]).astype(f32)).astype(f32)
                       for c in range(3)], 1)
        ln, lm = np.sqrt(f32_dot(n_obj, n_obj)).astype(f32), np.sqrt(f32_dot(mm, mm)).astype(f32)
        ok = (lm != 0) & np.isfinite(lm)
        scaled = (mm * (ln / np.where(ok, lm, f32(1))).astype(f32)[:, None]).astype(f32)
    n_world = np.where(ident[ids[hit]][:, None], n_obj, np.where(ok[:, None], scaled, mm)).astype(f32)
    d, o, t = rays["d"][hit], rays["o"][hit], hits["t"][hit]
    n = np.where((f32_dot(d, n_world) > 0)[:, None], -n_world, n_world)
    return hit, ((o + (d * t[:, None]).astype(f32)).astype(f32) + (n * f32(0.0002)).astype(f32)).astype(f32)


@pytest.mark.gpu
def test_v5_every_class_walks_with_its_own_mask(cr, ob, cornell, tess8):
    from caitlynrenderer_amd import tiles
    meshes, mats, light, M, mesh_of, masks = v5_scene(cr, cornell, tess8)
    inst = cr.InstancedScene(meshes, cr.instances_array(M, mesh_of, masks))
    W, H = 160, 96
    P = W * H
    cam = look_at(cr, (2.0, 3.0, 28.0), (0.0, 0.0, 0.0))
    sc = inst.frame_scene(shading_of(meshes), mats, light, W, H, 2)
    sc.update(cam)
    for name, value in masks_on(1, 2, 4) + (("count_visits", 1),):
        sc.set_option(name, value)
    rx, ry = RVS[0]
    sc.render_frame(rx, ry)
    st = sc.frame_stats()
    a = handle_arrays(inst)
    seg0 = primary_oracle(ob, cam, W, H).primary_rays(rx, ry, jitter=True)
    seg1, sh0, sh1 = sc.debug_read_queue(0, 1), sc.debug_read_queue(2, 0), sc.debug_read_queue(2, 1)
    assert min(seg1.shape[0], sh0.shape[0], sh1.shape[0]) > 0
    h0, i0, s0 = walk(ob, a, seg0, ob.CLOSEST, 1)
    h1, i1, s1 = walk(ob, a, seg1, ob.CLOSEST, 2)
    _, _, t0 = walk(ob, a, sh0, ob.ANY, 4)
    _, _, t1 = walk(ob, a, sh1, ob.ANY, 4)
    assert st["closest_rays"] == P + seg1.shape[0] and st["any_rays"] == sh0.shape[0] + sh1.shape[0]
    assert (st["nodes_closest"], st["tris_closest"]) == tuple(x + y for x, y in zip(counts(s0), counts(s1)))
    assert (st["nodes_any"], st["tris_any"]) == tuple(x + y for x, y in zip(counts(t0), counts(t1)))
    assert st["stack_overflows"] == 0
    # each class saw its own instances only, and the unmasked walk would have seen others
    assert ((masks[i0[i0 >= 0]] & 1) != 0).all() and ((masks[i1[i1 >= 0]] & 2) != 0).all()
    assert (walk(ob, a, seg0, ob.CLOSEST)[1] != i0).any() and (walk(ob, a, seg1, ob.CLOSEST)[1] != i1).any()
    # origins: segment 0's shadow rays and the path rays entering segment 1 start at the MASKED primary hits' points ...
    hit, point = world_hit_points(meshes, mesh_of, inst, seg0, h0, i0)
    want = {int(p): point[k] for k, p in enumerate(hit)}
    tl = tiles.shard_tiles_of_library(W, H, 16)
    dy, dx = tiles.pixel_grid(16)

    def pixel_of(path):
        tx, ty = tl[path // 256]
        return int((ty * 16 + dy[path % 256]) * W + tx * 16 + dx[path % 256])

    for q in (sh0, seg1):
        for e in q:
            p = pixel_of(int(e["pad"]))
            assert p in want and np.array_equal(e["o"].view(np.uint32), want[p].view(np.uint32)), (p, e["o"], want.get(p))
    assert seg1.shape[0] == hit.size                       # every Lambert hit bounces at max_depth 2
    # ... and segment 1's shadow rays at the masked bounce hits' points (a shadow entry's pad is its contribution slot: P + path)
    hit1, point1 = world_hit_points(meshes, mesh_of, inst, seg1, h1, i1)
    want1 = {int(seg1["pad"][p]): point1[k] for k, p in enumerate(hit1)}
    for e in sh1:
        path = int(e["pad"]) - P
        assert path in want1 and np.array_equal(e["o"].view(np.uint32), want1[path].view(np.uint32)), (path, e["o"], want1.get(path))
    close(inst, sc)


# ---------------------------------------------------------------- option refusals ----

@pytest.mark.gpu
def test_mask_options_refuse_what_is_out_of_range_and_flat_scenes(cr, ob, cornell):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    mesh, cam = cornell
    meshes, _ = split_mesh(cr, mesh, 4)
    inst, sc = identity_scene(cr, meshes, mesh, cam, 67, 45, 3, masks=np.array([1, 2, 1, 1]), options=masks_on(1, 1, 1))
    frames(sc, 2)
    before = sc.read_sum()
    for name, value in ((b"instance_masks", 2), (b"instance_masks", -1), (b"mask_primary", 256), (b"mask_bounce", -1), (b"mask_shadow", 1 << 16),
                        (b"mask_shadow", 256)):
        assert L.crt_set_option(sc._h, name, value) == _lib.CRT_ERR_INVALID, (name, value)
        assert len(L.crt_last_error()) > 20
    assert_same_bits(sc.read_sum(), before)
    sc.reset()
    frames(sc, 2)
    assert_same_bits(sc.read_sum(), before)                # the refused values changed no option
    for name, value in masks_on(0, 255, 0):                # the whole range is accepted
        sc.set_option(name, value)
    close(inst, sc)
    flat = cr.Scene(cr.SceneData.build(mesh, cam), 67, 45, 3)
    frames(flat, 2)
    before = flat.read_sum()
    for name in (b"instance_masks", b"mask_primary", b"mask_bounce", b"mask_shadow"):
        assert L.crt_set_option(flat._h, name, 1) == _lib.CRT_ERR_INVALID, name
        assert b"unknown option" in L.crt_last_error()
    assert_same_bits(flat.read_sum(), before)
    flat.close()
