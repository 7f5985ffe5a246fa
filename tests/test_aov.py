"""First-hit feature buffers (crt_render_aov): depth, ids, shading normal, albedo and emission of a frame's primary hits,
held bit for bit to the CPU oracle's hits (Oracle.primary_rays + Oracle.trace, ob.trace_instances on the handle's debug reads) and a
float32 numpy restatement of the attribute fetch (the normal as test_general_transforms_normal_and_hit_point writes it, the texture
filter as oracle.c's sample_albedo, pow in float64 rounded once).

CPU: the ABI and the Python surface (C1, C2), and the premises the GPU checks rest on (C3).  GPU: flat scenes (G1), channel subsets (G2),
identity instances against the flat reference (G3), general transforms with offsets across a refit and a set (G4), masks (G5), shards
(G6), nothing else moves (G7), refusals and lifetime (G8).  All pixels are compared; the only tolerance is the textured ALBEDO's: the
expected number of unequal pixels is 0, any that occur must be within 1 float32 ulp, and their count is printed."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from test_instances_frames import (RVS, blas_roots, device_walk, emissive_meshes, f32_dot, flat_variants, look_at, mesh_of_instances, primary_oracle,
                                   shading_of, split_mesh)
from test_instances_oracle import IDENTITY, host_blas, host_scene, is_identity, orc, placed_instances

f32 = np.float32
THREADS = 16
SIZES = ((67, 45), (231, 130))
NAMES = ["cornell", "textured", "tess8_mat"]
MISS_T = f32(1e9)
CHANNELS = ("HIT", "IDS", "NORMAL", "ALBEDO", "EMISSION")


def bit_of(cr, name):
    return getattr(cr, "AOV_" + name)


# ---------------------------------------------------------------- the reference: numpy float32 on the oracle's hits ----

def sample_albedo_np(textures, u, v, layer):
    """oracle.c sample_albedo: GL_LINEAR, GL_REPEAT over texels c / 255.0f; float32, no fma"""
    L, H, W, _ = textures.shape
    img = textures.astype(f32) / f32(255.0)
    layer = np.clip(layer, 0, L - 1)
    x, y = u * f32(W) - f32(0.5), v * f32(H) - f32(0.5)
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    bx, by = ~(np.abs(x0) < f32(1e9)), ~(np.abs(y0) < f32(1e9))
    x0, fx = np.where(bx, f32(0), x0), np.where(bx, f32(0), fx)
    y0, fy = np.where(by, f32(0), y0), np.where(by, f32(0), fy)
    i0, i1 = np.mod(x0.astype(np.int64), W), np.mod(x0.astype(np.int64) + 1, W)
    j0, j1 = np.mod(y0.astype(np.int64), H), np.mod(y0.astype(np.int64) + 1, H)
    t00, t10, t01, t11 = img[layer, j0, i0], img[layer, j0, i1], img[layer, j1, i0], img[layer, j1, i1]
    fx, fy = fx[:, None].astype(f32), fy[:, None].astype(f32)
    top = t00 * (f32(1.0) - fx) + t10 * fx
    bot = t01 * (f32(1.0) - fx) + t11 * fx
    out = top * (f32(1.0) - fy) + bot * fy
    assert out.dtype == f32
    return out


def shading(tris, mtl, normals, texcoords, materials, textures, bu, bv, d, w2o=None, general=None):
    """the channels' values of n hits: tris (n, 12) the hit triangles' rows, mtl (n) the material indices the integrator reads, d the ray
    directions; w2o (n, 3, 4) / general (n): the hit instances' world_to_object and whether they take the general path"""
    bu, bv, d = bu.astype(f32), bv.astype(f32), d.astype(f32)
    w = (f32(1.0) - bu) - bv
    flat = tris[:, 7] == 0
    N = normals if normals.shape[0] else np.zeros((1, 3), f32)
    vn = np.where(flat[:, None], 0, tris[:, 4:7])
    na, nb, nc = N[vn[:, 0]], N[vn[:, 1]], N[vn[:, 2]]
    interp = (na * w[:, None] + nb * bu[:, None]) + nc * bv[:, None]
    n_obj = np.where(flat[:, None], tris[:, 4:7].astype(f32), interp).astype(f32)
    n_w = n_obj
    if w2o is not None:
        with np.errstate(all="ignore"):
            mm = np.stack([(w2o[:, 0, c] * n_obj[:, 0] + w2o[:, 1, c] * n_obj[:, 1]) + w2o[:, 2, c] * n_obj[:, 2] for c in range(3)], 1).astype(f32)
            ln, lm = np.sqrt(f32_dot(n_obj, n_obj)).astype(f32), np.sqrt(f32_dot(mm, mm)).astype(f32)
            ok = (lm != 0) & np.isfinite(lm)
            scaled = (mm * (ln / np.where(ok, lm, f32(1))).astype(f32)[:, None]).astype(f32)
        n_w = np.where(general[:, None], np.where(ok[:, None], scaled, mm), n_obj).astype(f32)
    flip = f32_dot(d, n_w) > 0
    normal = np.where(flip[:, None], -n_w, n_w).astype(f32)
    tex = materials[mtl, 12]
    textured = (tex != -1) & (textures is not None)
    albedo = materials[mtl, 0:3].astype(f32).copy()
    outside = 0
    if textured.any():
        k = np.nonzero(textured)[0]
        vt = tris[k, 8:11]
        ta, tb, tc = texcoords[vt[:, 0]], texcoords[vt[:, 1]], texcoords[vt[:, 2]]
        tu = (ta[:, 0] * w[k] + tb[:, 0] * bu[k]) + tc[:, 0] * bv[k]
        tv = (ta[:, 1] * w[k] + tb[:, 1] * bu[k]) + tc[:, 1] * bv[k]
        assert tu.dtype == f32 and tv.dtype == f32
        outside = int(((tu < 0) | (tu >= 1) | (tv < 0) | (tv >= 1)).sum())
        c = sample_albedo_np(textures, tu, tv, tex[k].astype(np.int64))
        albedo[k] = np.power(c.astype(np.float64), np.float64(f32(2.2))).astype(f32)
    emissive = materials[mtl, 7] != -1
    emission = np.where(emissive[:, None], materials[mtl, 4:7], f32(0)).astype(f32)
    flags = flip.astype(np.int32) | (emissive.astype(np.int32) << 1) | (textured.astype(np.int32) << 2)
    assert normal.dtype == f32 and albedo.dtype == f32
    return dict(normal=normal, albedo=albedo, emission=emission, flags=flags, flip=flip, emissive=emissive, textured=textured,
                layer=np.where(textured, tex, -1).astype(np.int64), outside=outside)


def frame_of(cr, W, H, idx, t, u, v, tri, inst, mesh, mtl, sh):
    """the five channels of a W x H frame whose pixels `idx` (py * W + px) hit; every other pixel holds the miss values"""
    hit = np.zeros(H * W, cr.HIT_DT)
    hit["t"], hit["tri"] = MISS_T, -1
    ids = np.zeros(H * W, cr.AOV_IDS_DT)
    ids["instance"] = ids["mesh"] = ids["material"] = -1
    hit["t"][idx], hit["u"][idx], hit["v"][idx], hit["tri"][idx] = t, u, v, tri
    ids["instance"][idx], ids["mesh"][idx], ids["material"][idx], ids["flags"][idx] = inst, mesh, mtl, sh["flags"]
    out = {"HIT": hit.reshape(H, W), "IDS": ids.reshape(H, W)}
    for name in ("normal", "albedo", "emission"):
        a = np.zeros((H * W, 4), f32)
        a[idx, :3] = sh[name]
        out[name.upper()] = a.reshape(H, W, 4)
    out["textured"] = np.zeros(H * W, bool)
    out["textured"][idx] = sh["textured"]
    return out


def words(a):
    """(pixels, 4) uint32: a channel's bytes"""
    return np.ascontiguousarray(a).view(np.uint32).reshape(-1, 4)


def read_all(cr, sc):
    return {name: sc.read_aov(bit_of(cr, name)) for name in CHANNELS}


def assert_channels(cr, got, want, what=(), names=CHANNELS):
    """by bytes; on textured pixels ALBEDO may differ by 1 float32 ulp (expected count 0, printed).  Returns that count"""
    unequal = 0
    for name in names:
        g, w = words(got[name]), words(want[name])
        bad = np.nonzero((g != w).any(1))[0]
        if name == "ALBEDO" and bad.size:
            tex = want["textured"][bad]
            assert tex.all(), (what, name, "untextured pixels differ", bad[~tex][:4], got[name].reshape(-1, 4)[bad[~tex][:4]], want[name].reshape(-1, 4)[bad[~tex][:4]])
            gi, wi = g[bad].astype(np.int64), w[bad].astype(np.int64)          # positive floats: the distance in ulps is the difference of the words
            assert (np.abs(gi - wi) <= 1).all(), (what, "textured ALBEDO beyond 1 ulp", bad[:4], got[name].reshape(-1, 4)[bad[:4]], want[name].reshape(-1, 4)[bad[:4]])
            unequal += bad.size
            continue
        assert bad.size == 0, (what, name, bad.size, bad[:4], g[bad[:4]], w[bad[:4]])
    return unequal


_FLAT = {}


def flat_data(cr, mesh, cam, builder):
    """the SceneData the oracle walks: the host SBVH (spatial splits: duplicates), or the device builder's tree"""
    if builder == "sbvh":
        return cr.SceneData.build(mesh, cam)
    return cr.SceneData.build(mesh, cam, builder=builder, convert="device")


def flat_reference(cr, ob, name, builder, mesh, data, cam, W, H, rv, jitter):
    """the five channels of the flat scene's view, computed once per case"""
    key = (name, builder, W, H, rv, jitter)
    if key not in _FLAT:
        o = ob.Oracle(data, W, H, 1, camera=cam)
        rays = o.primary_rays(rv[0], rv[1], jitter=bool(jitter))
        h = o.trace(rays, ob.BVH8, ob.CLOSEST, ob.TIE_LOWEST_ID, threads=THREADS)
        idx = np.nonzero(h["tri"] >= 0)[0]
        tri = h["tri"][idx]
        rows = mesh.triangles[tri]
        mtl = rows[:, 3]
        sh = shading(rows, mtl, mesh.normals, mesh.texcoords, mesh.materials, getattr(mesh, "albedo_textures", None), h["u"][idx], h["v"][idx], rays["d"][idx])
        ref = frame_of(cr, W, H, idx, h["t"][idx], h["u"][idx], h["v"][idx], tri, 0, 0, mtl, sh)
        ref["sh"], ref["idx"] = sh, idx
        _FLAT[key] = ref
    return _FLAT[key]


def instanced_reference(cr, W, H, rays, hits, ids, meshes, mesh_of, offs, materials, textures, w2o, ident):
    """the five channels from a two-level walk's (hits, instance ids)"""
    idx = np.nonzero(ids >= 0)[0]
    i = ids[idx]
    m = np.asarray(mesh_of)[i]
    tri, bu, bv = hits["tri"][idx], hits["u"][idx], hits["v"][idx]
    mtl = np.zeros(idx.size, np.int64)
    sh = None
    for q, mesh in enumerate(meshes):
        sel = np.nonzero(m == q)[0]
        rows = mesh.triangles[tri[sel]]
        mt = rows[:, 3].astype(np.int64) + np.asarray(offs, np.int64)[i[sel]]
        part = shading(rows, mt, mesh.normals, mesh.texcoords, materials, textures, bu[sel], bv[sel], rays["d"][idx][sel], w2o[i[sel]], ~ident[i[sel]])
        if sh is None:
            sh = {k: np.zeros((idx.size,) + v.shape[1:], v.dtype) for k, v in part.items() if isinstance(v, np.ndarray)}
        for k in sh:
            sh[k][sel] = part[k]
        mtl[sel] = mt
    ref = frame_of(cr, W, H, idx, hits["t"][idx], bu, bv, tri, i, m, mtl, sh)
    ref["sh"], ref["idx"], ref["inst"], ref["mesh"], ref["mtl"] = sh, idx, i, m, mtl
    return ref


# ---------------------------------------------------------------- the general-transform scene of G4 / G5 ----

SEED_G = 431
W4, H4 = 160, 96


def table_of(mats):
    """emissive_meshes' six Lambert materials + five emissive ones (distinct albedos and emissions, the scene's one light): a material offset
    can take a triangle to either kind"""
    rng = np.random.default_rng(79)
    extra = np.repeat(mats[:1], 5, 0)
    extra[:, 0:3] = rng.uniform(0.2, 0.9, (5, 3))
    extra[:, 4:7] = rng.uniform(0.1, 4.0, (5, 3))
    extra[:, 7] = 0
    return np.concatenate([mats, extra]).astype(f32)


def offsets_for(rng, meshes, mesh_of, n_materials):
    hi = np.array([int(m.triangles[:, 3].max()) for m in meshes])
    return rng.integers(0, n_materials - hi[mesh_of]).astype(np.uint32)


def general_scene(cr, cornell, tess8):
    """120 placed instances (rotations, scales 0.5 - 2, mirrors) of emissive_meshes' three meshes, one translated identity, one bitwise
    identity, random in-range material offsets, masks that hide every second instance from ray mask 1"""
    meshes, mats, light = emissive_meshes(cr, cornell, tess8, lambert=True)
    table = table_of(mats)
    rng = np.random.default_rng(SEED_G)
    M, mesh_of = placed_instances(rng, 120, 3, spread=9.0)
    mesh_of[:3] = (0, 1, 2)
    M[5] = np.concatenate([np.eye(3), [[-4.0], [-1.0], [12.0]]], 1)        # a translated identity, in front of the others: the general path with W = I
    M[6] = IDENTITY                                                         # a bitwise identity: the flagged path
    mesh_of[5], mesh_of[6] = 1, 0
    offs = offsets_for(rng, meshes, mesh_of, table.shape[0])
    masks = np.where(np.arange(120) % 2 == 0, 2, 1)
    return dict(meshes=meshes, table=table, light=light, rng=rng, M=M, mesh_of=mesh_of, offs=offs, masks=masks)


def camera_g(cr):
    return look_at(cr, (2.0, 3.0, 30.0), (0.0, 0.0, 0.0))


# ---------------------------------------------------------------- C1, C2 ----

def test_c1_the_library_exports_the_entries_and_refuses_null_scenes(cr):
    from caitlynrenderer_amd import _lib
    L = _lib.lib()
    for name in ("crt_render_aov", "crt_read_aov", "crt_aov_device"):
        assert name in _lib.SYMBOLS and hasattr(L, name)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "crt.h")).read()
    enum = dict(re.findall(r"CRT_AOV_(\w+) = (\d+)", header))
    assert set(enum) == {"HIT", "IDS", "NORMAL", "ALBEDO", "EMISSION", "ALL"}
    for name, value in enum.items():
        assert getattr(cr, "AOV_" + name) == int(value) == getattr(_lib, "CRT_AOV_" + name)
    assert (cr.AOV_HIT, cr.AOV_IDS, cr.AOV_NORMAL, cr.AOV_ALBEDO, cr.AOV_EMISSION, cr.AOV_ALL) == (1, 2, 4, 8, 16, 31)
    buf = np.zeros(16, np.uint8)
    p = C.c_void_p()
    assert L.crt_render_aov(None, 0.0, 0.0, cr.AOV_ALL, 1) == _lib.CRT_ERR_INVALID
    assert L.crt_read_aov(None, cr.AOV_HIT, buf.ctypes.data_as(C.c_void_p), 16) == _lib.CRT_ERR_INVALID
    assert L.crt_aov_device(None, cr.AOV_HIT, C.byref(p)) == _lib.CRT_ERR_INVALID and not p.value


def test_c2_the_scene_methods_and_their_dtypes(cr):
    for name in ("render_aov", "read_aov", "aov_device"):
        assert callable(getattr(cr.Scene, name))
    ids = np.dtype([("instance", "<i4"), ("mesh", "<i4"), ("material", "<i4"), ("flags", "<i4")])
    table = {cr.AOV_HIT: (cr.HIT_DT, ()), cr.AOV_IDS: (ids, ()), cr.AOV_NORMAL: (np.dtype("<f4"), (4,)), cr.AOV_ALBEDO: (np.dtype("<f4"), (4,)),
             cr.AOV_EMISSION: (np.dtype("<f4"), (4,))}
    assert cr.AOV_IDS_DT == ids and cr.AOV_IDS_DT.itemsize == 16 and cr.HIT_DT.itemsize == 16
    assert set(cr.AOV_DTYPES) == set(table)
    for ch, (dt, tail) in table.items():
        got_dt, got_tail = cr.AOV_DTYPES[ch]
        assert np.dtype(got_dt) == dt and tuple(got_tail) == tail
        assert np.dtype(got_dt).itemsize * int(np.prod(tail, dtype=np.int64)) == 16          # 16 bytes per pixel, every channel
    import inspect
    sig = inspect.signature(cr.Scene.render_aov)
    assert [p for p in sig.parameters] == ["self", "rx", "ry", "channels", "sync"]
    assert (sig.parameters["rx"].default, sig.parameters["ry"].default, sig.parameters["channels"].default, sig.parameters["sync"].default) == (0.0, 0.0, cr.AOV_ALL, True)


# ---------------------------------------------------------------- C3: premises, on the oracle ----

@pytest.mark.parametrize("name", NAMES)
def test_c3a_the_flat_views_are_not_pictures_of_the_sky(cr, ob, cornell, textured, name):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    data = flat_data(cr, mesh, cam, "sbvh")
    for W, H in SIZES:
        for rv in RVS[:3]:
            ref = flat_reference(cr, ob, name, "sbvh", mesh, data, cam, W, H, rv, 1)
            share = ref["idx"].size / (W * H)
            print(f"C3a {name} {W}x{H} rv {rv}: {share:.3f} of the pixels hit")
            assert share >= 0.2


def test_c3b_the_textured_view_shows_both_layers_the_untextured_rest_and_a_wrap(cr, ob, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    data = flat_data(cr, mesh, cam, "sbvh")
    for W, H in SIZES:
        for rv in RVS[:3]:
            sh = flat_reference(cr, ob, "textured", "sbvh", mesh, data, cam, W, H, rv, 1)["sh"]
            counts = [int((sh["layer"] == 0).sum()), int((sh["layer"] == 1).sum()), int((~sh["textured"]).sum())]
            print(f"C3b {W}x{H} rv {rv}: layer 0 / layer 1 / untextured hit pixels {counts}, texcoords outside [0, 1): {sh['outside']}")
            assert min(counts) >= 200 and sh["outside"] >= 1


def general_premises(ref, g, M, mesh_of, offs):
    sh, inst, mesh = ref["sh"], ref["inst"], ref["mesh"]
    ident_like = (inst == 5) | (inst == 6)
    det = np.linalg.det(np.asarray(M, np.float64)[:, :, :3])
    looks = [len(set(np.asarray(offs)[inst[mesh == q]].tolist())) for q in range(3)]
    return dict(flipped=int(sh["flip"].sum()), unflipped=int((~sh["flip"]).sum()), identity=int(ident_like.sum()), general=int((~ident_like).sum()),
                mirrored=int((det[inst] < 0).sum()), looks=looks, emissive=int(sh["emissive"].sum()), lambert=int((~sh["emissive"]).sum()))


def check_general_premises(p):
    assert p["flipped"] >= 500 and p["unflipped"] >= 500, p
    assert p["identity"] >= 100 and p["general"] >= 1000, p
    assert p["mirrored"] >= 1, p
    assert min(p["looks"]) >= 3, p
    assert p["emissive"] >= 1 and p["lambert"] >= 1, p


def test_c3c_the_general_transform_view_reaches_every_path(cr, ob, cornell, tess8):
    """on the arrays of the same instances assembled on the host: the closest hit is the minimum of (t, instance, id), whatever the tree"""
    g = general_scene(cr, cornell, tess8)
    s = host_scene(cr, [host_blas(cr, m) for m in g["meshes"]], list(g["M"]), list(g["mesh_of"]))
    rays = primary_oracle(ob, camera_g(cr), W4, H4).primary_rays(*RVS[0], jitter=True)
    hits, ids, _, _, refused = orc(ob, s, rays)
    assert refused.sum() == 0
    w2o = np.array([cr.instance_inverse(m) for m in g["M"]], f32).reshape(-1, 3, 4)
    ident = np.array([is_identity(m) for m in g["M"]])
    ref = instanced_reference(cr, W4, H4, rays, hits, ids, g["meshes"], g["mesh_of"], g["offs"], g["table"], None, w2o, ident)
    p = general_premises(ref, g, g["M"], g["mesh_of"], g["offs"])
    print("C3c", p)
    check_general_premises(p)
    # G5: the masked walk (ray mask 1: the even instances are hidden) shows another picture
    r = rays.copy()
    r["pad"] = 1
    s_m = host_scene(cr, [host_blas(cr, m) for m in g["meshes"]], list(g["M"]), list(g["mesh_of"]), masks=g["masks"])
    _, ids_m, _, _, _ = orc(ob, s_m, r, masked=True)
    differ = int((ids_m != ids).sum())
    print("C3c masked walk: pixels whose instance differs", differ)
    assert differ >= 100 and (ids_m[ids_m >= 0] % 2 == 1).all()


# ---------------------------------------------------------------- G1: flat scenes ----

def flat_scene(cr, mesh, cam, builder, W, H, depth=1):
    if builder == "sbvh":
        return cr.Scene(cr.SceneData.build(mesh, cam), W, H, depth)
    return cr.Scene(cr.SceneData.for_device_build(mesh, cam, builder=builder), W, H, depth)


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sbvh", "sah"])
@pytest.mark.parametrize("name", NAMES)
def test_g1_flat_scenes_bit_for_bit(cr, ob, cornell, textured, name, builder):
    mesh, _ = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    data = flat_data(cr, mesh, cam, builder)
    unequal = 0
    for W, H in SIZES:
        sc = flat_scene(cr, mesh, cam, builder, W, H)
        for jitter in (0, 1):
            sc.set_option("jitter", jitter)
            for rv in RVS[:3]:
                ref = flat_reference(cr, ob, name, builder, mesh, data, cam, W, H, rv, jitter)
                sc.render_aov(rv[0], rv[1])
                unequal += assert_channels(cr, read_all(cr, sc), ref, (name, builder, W, H, jitter, rv))
        sc.close()
    print(f"G1 {name} {builder}: textured ALBEDO pixels that differ from libm's pow by 1 ulp: {unequal}")


# ---------------------------------------------------------------- G2: channel subsets ----

@pytest.mark.gpu
def test_g2_a_subset_renders_its_channels_and_leaves_the_others(cr, ob, cornell, textured):
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    data = flat_data(cr, mesh, cam, "sbvh")
    W, H = SIZES[1]
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H)
    first, second = (flat_reference(cr, ob, "textured", "sbvh", mesh, data, cam, W, H, rv, 1) for rv in RVS[:2])
    sc.render_aov(*RVS[0], channels=cr.AOV_HIT | cr.AOV_IDS)
    assert_channels(cr, {n: sc.read_aov(bit_of(cr, n)) for n in ("HIT", "IDS")}, first, "subset first", ("HIT", "IDS"))
    for n in ("NORMAL", "ALBEDO", "EMISSION"):               # never rendered: refused
        with pytest.raises(CrtError) as e:
            sc.read_aov(bit_of(cr, n))
        assert e.value.code == CRT_ERR_INVALID
        with pytest.raises(CrtError) as e:
            sc.aov_device(bit_of(cr, n))
        assert e.value.code == CRT_ERR_INVALID
    sc.render_aov(*RVS[0])
    assert_channels(cr, read_all(cr, sc), first, "all")
    sc.render_aov(*RVS[1], channels=cr.AOV_HIT | cr.AOV_IDS)
    got = read_all(cr, sc)
    assert (words(first["HIT"]) != words(second["HIT"])).any()
    assert_channels(cr, got, second, "subset second", ("HIT", "IDS"))
    assert_channels(cr, got, first, "kept", ("NORMAL", "ALBEDO", "EMISSION"))
    sc.close()


# ---------------------------------------------------------------- G3: identity instances of a split flat scene ----

def identity_scene(cr, mesh, parts, builder, W, H, depth=1):
    meshes, first = split_mesh(cr, mesh, parts)
    inst = cr.InstancedScene(meshes, cr.instances_array([IDENTITY] * parts, np.arange(parts)), builder=builder)
    sc = inst.frame_scene(shading_of(meshes), mesh.materials, mesh.lights, W, H, depth, textures=getattr(mesh, "albedo_textures", None))
    return inst, sc, first


def split_reference(ref, first):
    """the flat reference with the ids of the split: instance = mesh = the part, HIT.tri = the id within the part"""
    out = dict(ref)
    hit, ids = ref["HIT"].copy().reshape(-1), ref["IDS"].copy().reshape(-1)
    idx = ref["idx"]
    part = np.searchsorted(first, hit["tri"][idx], side="right") - 1
    hit["tri"][idx] -= first[part].astype(np.int32)
    ids["instance"][idx] = ids["mesh"][idx] = part
    out["HIT"], out["IDS"] = hit.reshape(ref["HIT"].shape), ids.reshape(ref["IDS"].shape)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("builder", ["sah", "lbvh"])
@pytest.mark.parametrize("name", NAMES)
def test_g3_identity_instances_give_the_flat_scenes_buffers(cr, ob, cornell, textured, name, builder):
    mesh, parts = flat_variants(cr, cornell, textured)[name]
    cam = cornell[1]
    data = flat_data(cr, mesh, cam, "sbvh")
    unequal = 0
    for W, H in SIZES:
        inst, sc, first = identity_scene(cr, mesh, parts, builder, W, H)
        sc.update(cam)
        assert (inst.instance_records()[:, 14].view(np.uint32) == 1).all()
        for rv in RVS[:3]:
            ref = split_reference(flat_reference(cr, ob, name, "sbvh", mesh, data, cam, W, H, rv, 1), first)
            sc.render_aov(rv[0], rv[1])
            unequal += assert_channels(cr, read_all(cr, sc), ref, (name, builder, W, H, rv))
        sc.close()
        inst.close()
    print(f"G3 {name} {builder}: textured ALBEDO pixels 1 ulp off: {unequal}")


# ---------------------------------------------------------------- G4, G5: general transforms, masks ----

def handle_reference(cr, ob, inst, g, M, mesh_of, offs, cam, rv, ray_mask=None):
    rays = primary_oracle(ob, cam, W4, H4).primary_rays(rv[0], rv[1], jitter=True)
    if ray_mask is None:
        hits, ids, _, _, refused = device_walk(ob, inst, rays)
    else:
        r = rays.copy()
        r["pad"] = ray_mask
        info = inst.info()
        hits, ids, _, _, refused = ob.trace_instances(inst.tlas_nodes(), inst.instance_records(), inst.blas_nodes(), inst.blas_records(), r,
                                                      info["tlas_bytes"] // 80, info["stack_entries"], ob.CLOSEST | ob.INSTANCE_MASK, threads=THREADS)
    assert refused.sum() == 0
    rec = inst.instance_records()
    ident = np.zeros(rec.shape[0], bool)
    ident[rec[:, 13].view(np.uint32)] = rec[:, 14].view(np.uint32) != 0
    assert np.array_equal(mesh_of_instances(inst, blas_roots(inst, 3)), np.asarray(mesh_of))
    w2o = inst.world_to_object().reshape(-1, 3, 4)
    return instanced_reference(cr, W4, H4, rays, hits, ids, g["meshes"], mesh_of, offs, g["table"], None, w2o, ident)


def general_handle(cr, cornell, tess8):
    g = general_scene(cr, cornell, tess8)
    inst = cr.InstancedScene(g["meshes"], cr.instances_array(g["M"], g["mesh_of"], g["masks"], g["offs"]), capacity=300)
    sc = inst.frame_scene(shading_of(g["meshes"]), g["table"], g["light"], W4, H4, 1)
    cam = camera_g(cr)
    sc.update(cam)
    return g, inst, sc, cam


@pytest.mark.gpu
def test_g4_general_transforms_across_a_refit_and_a_set(cr, ob, cornell, tess8):
    g, inst, sc, cam = general_handle(cr, cornell, tess8)
    rng = g["rng"]
    ref = handle_reference(cr, ob, inst, g, g["M"], g["mesh_of"], g["offs"], cam, RVS[0])
    check_general_premises(general_premises(ref, g, g["M"], g["mesh_of"], g["offs"]))
    sc.render_aov(*RVS[0])
    assert_channels(cr, read_all(cr, sc), ref, "created")
    # a refit that moves every instance and changes offsets: seen by the next call, no crt_reset, no re-create
    M2 = g["M"].copy()
    M2[:, :, 3] += rng.uniform(-1.5, 1.5, (120, 3)).astype(f32)
    offs2 = offsets_for(rng, g["meshes"], g["mesh_of"], g["table"].shape[0])
    assert (offs2 != g["offs"]).mean() > 0.5
    inst.refit(cr.instances_array(M2, g["mesh_of"], g["masks"], offs2))
    ref2 = handle_reference(cr, ob, inst, g, M2, g["mesh_of"], offs2, cam, RVS[1])
    sc.render_aov(*RVS[1])
    got2 = read_all(cr, sc)
    assert_channels(cr, got2, ref2, "refitted")
    assert (words(got2["IDS"]) != words(ref["IDS"])).any()
    # a set to another count
    M3, mesh_of3 = placed_instances(rng, 260, 3, spread=9.0)
    mesh_of3[:3] = (0, 1, 2)
    offs3 = offsets_for(rng, g["meshes"], mesh_of3, g["table"].shape[0])
    inst.set(cr.instances_array(M3, mesh_of3, material_offsets=offs3))
    ref3 = handle_reference(cr, ob, inst, g, M3, mesh_of3, offs3, cam, RVS[2])
    sc.render_aov(*RVS[2])
    assert_channels(cr, read_all(cr, sc), ref3, "set")
    sc.close()
    inst.close()


@pytest.mark.gpu
def test_g5_the_masked_walk_with_mask_primary(cr, ob, cornell, tess8):
    g, inst, sc, cam = general_handle(cr, cornell, tess8)
    plain = handle_reference(cr, ob, inst, g, g["M"], g["mesh_of"], g["offs"], cam, RVS[0])
    masked = handle_reference(cr, ob, inst, g, g["M"], g["mesh_of"], g["offs"], cam, RVS[0], ray_mask=1)
    for name, value in (("instance_masks", 1), ("mask_primary", 1), ("mask_bounce", 255), ("mask_shadow", 255)):
        sc.set_option(name, value)
    sc.render_aov(*RVS[0])
    got = read_all(cr, sc)
    assert_channels(cr, got, masked, "masked")
    differ = (words(got["IDS"]) != words(plain["IDS"])).any(1) | (words(got["HIT"]) != words(plain["HIT"])).any(1)
    assert differ.sum() >= 100, differ.sum()
    seen = got["IDS"]["instance"]
    assert (seen[seen >= 0] % 2 == 1).all()
    sc.set_option("instance_masks", 0)
    sc.render_aov(*RVS[0])
    assert_channels(cr, read_all(cr, sc), plain, "option back to 0")
    sc.close()
    inst.close()


# ---------------------------------------------------------------- G6: shards ----

def miss_frame(cr, W, H):
    return frame_of(cr, W, H, np.zeros(0, np.int64), 0, 0, 0, 0, 0, 0, 0, dict(flags=0, normal=0, albedo=0, emission=0, textured=False))


def check_shards(cr, make, ref, W, H):
    """every pixel holds the one-rank value in the rank that owns it and the miss value in the other; the union is the one-rank result"""
    from caitlynrenderer_amd import tiles
    miss = miss_frame(cr, W, H)
    union = {n: miss[n].copy() for n in CHANNELS}
    covered = np.zeros((H, W), np.int64)
    for rank in (0, 1):
        sc, closer = make()
        sc.set_shard(rank, 2, 16)
        sc.render_aov(*RVS[0])
        got = read_all(cr, sc)
        closer()
        own = np.zeros((H, W), bool)
        for tx, ty in tiles.shard_tiles_of_library(W, H, 16, rank, 2):
            own[ty * 16:ty * 16 + 16, tx * 16:tx * 16 + 16] = True
        covered += own
        shown = {}
        for n in CHANNELS:
            elsewhere = ~own.reshape(-1)
            assert (words(got[n])[elsewhere] == words(miss[n])[elsewhere]).all(), (n, rank)
            shown[n] = got[n].copy()
            shown[n][~own] = ref[n][~own]                  # the rank's own pixels in the reference's frame
            union[n][own] = got[n][own]
        assert_channels(cr, shown, ref, ("shard", rank))
    assert (covered == 1).all()
    sc, closer = make()
    sc.render_aov(*RVS[0])
    one = read_all(cr, sc)
    closer()
    for n in CHANNELS:
        assert np.array_equal(words(union[n]), words(one[n])), n


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g6_two_shard_ranks_fill_their_own_pixels(cr, ob, cornell, textured, kind):
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[1]
    data = flat_data(cr, mesh, cam, "sbvh")
    ref = flat_reference(cr, ob, "textured", "sbvh", mesh, data, cam, W, H, RVS[0], 1)
    if kind == "flat":
        def make():
            sc = flat_scene(cr, mesh, cam, "sbvh", W, H)
            return sc, sc.close
    else:
        first = split_mesh(cr, mesh, parts)[1]
        ref = split_reference(ref, first)

        def make():
            inst, sc, _ = identity_scene(cr, mesh, parts, "sah", W, H)
            sc.update(cam)
            return sc, lambda: (sc.close(), inst.close())
    check_shards(cr, make, ref, W, H)


# ---------------------------------------------------------------- G7: nothing else moves ----

# Which rays share a wave in a bounce segment follows the order in which the waves of the segment before appended to its queue (one atomic
# per wave): the lane-level counts do not depend on it, the wave-level step counts do, from one run of the same frames to the next.  So
# the whole record is compared where nothing is queued between launches (max_depth 1), and all of it but these four on three segments.
QUEUE_ORDER_FIELDS = ("wave_steps_closest_nodes", "wave_steps_closest_tris", "wave_steps_any_nodes", "wave_steps_any_tris")


def frames_state(sc, depth):
    st = sc.frame_stats()
    if depth > 1:
        st = {k: v for k, v in st.items() if k not in QUEUE_ORDER_FIELDS}
    return sc.read_sum(), st, sc.frame_count


@pytest.mark.gpu
@pytest.mark.parametrize("depth", [1, 3])
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g7_a_call_between_frames_changes_no_sum_count_or_stats(cr, ob, cornell, textured, kind, depth):
    mesh, parts = flat_variants(cr, cornell, textured)["tess8_mat"]
    cam = cornell[1]
    W, H = SIZES[1]

    def make():
        if kind == "flat":
            sc = flat_scene(cr, mesh, cam, "sbvh", W, H, depth)
            closer = sc.close
        else:
            inst, sc, _ = identity_scene(cr, mesh, parts, "sah", W, H, depth)
            sc.update(cam)
            closer = lambda: (sc.close(), inst.close())
        sc.set_option("count_visits", 1)
        return sc, closer

    plain, close_plain = make()
    for rv in RVS[:5]:
        plain.render_frame(*rv)
    want_sum, want_stats, want_count = frames_state(plain, depth)
    close_plain()
    sc, closer = make()
    for rv in RVS[:3]:
        sc.render_frame(*rv)
    stats3 = sc.frame_stats()
    sc.render_aov(*RVS[3])                                   # its own (rx, ry) is the next frame's: that frame's RNG state is its own all the same
    aov = read_all(cr, sc)
    assert sc.frame_stats() == stats3                        # the last frame's record, every field
    for rv in RVS[3:5]:
        sc.render_frame(*rv)
    got_sum, got_stats, got_count = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats and got_count == want_count
    assert got_stats["closest_rays"] > 0 and got_stats["nodes_closest"] > 0
    closer()
    # enqueued without a host wait behind asynchronous frames, a frame behind it: both give the synchronous results
    sc, closer = make()
    sc.render_frames(RVS[:3], sync=False)
    sc.render_aov(*RVS[3], sync=False)
    for rv in RVS[3:5]:
        sc.render_frame(*rv, sync=False)
    sc.sync()
    assert_channels(cr, read_all(cr, sc), dict(aov, textured=np.zeros(H * W, bool)), "async")
    got_sum, got_stats, _ = frames_state(sc, depth)
    assert np.array_equal(got_sum.view(np.uint32), want_sum.view(np.uint32))
    assert got_stats == want_stats
    closer()


# ---------------------------------------------------------------- G8: refusals and lifetime ----

def device_bytes_at(ptr, n):
    """n bytes at a device address, through the HIP runtime the library itself is linked to"""
    path = next(l.split()[-1] for l in open("/proc/self/maps") if "libamdhip64" in l)
    hip = C.CDLL(path)
    hip.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]
    hip.hipMemcpy.restype = C.c_int
    out = np.zeros(n, np.uint8)
    assert hip.hipMemcpy(out.ctypes.data_as(C.c_void_p), C.c_void_p(ptr), n, 2) == 0         # hipMemcpyDeviceToHost
    return out


@pytest.mark.gpu
def test_g8_refusals_leave_the_buffers_and_the_sum_as_they_were(cr, ob, cornell, textured):
    from caitlynrenderer_amd import _lib
    from caitlynrenderer_amd._lib import CRT_ERR_INVALID, CrtError
    mesh, _ = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[0]
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H)
    sc.render_frame(*RVS[0])
    sc.render_aov(*RVS[0])
    before, sum_before = read_all(cr, sc), sc.read_sum()

    def refused(call):
        with pytest.raises(CrtError) as e:
            call()
        assert e.value.code == CRT_ERR_INVALID, e.value
        assert str(e.value).split(": ", 1)[1]                 # crt_last_error says why

    L = _lib.lib()
    buf = np.zeros(W * H * 16, np.uint8)
    ptr = buf.ctypes.data_as(C.c_void_p)
    calls = [lambda: sc.render_aov(*RVS[1], channels=0), lambda: sc.render_aov(*RVS[1], channels=32), lambda: sc.render_aov(*RVS[1], channels=cr.AOV_HIT | 64),
             lambda: sc.aov_device(cr.AOV_HIT | cr.AOV_IDS), lambda: sc.aov_device(cr.AOV_ALL), lambda: sc.aov_device(0),
             lambda: _lib.check(L.crt_read_aov(sc._h, cr.AOV_HIT, ptr, W * H * 16 - 16)), lambda: _lib.check(L.crt_read_aov(sc._h, cr.AOV_HIT, ptr, W * H * 12)),
             lambda: _lib.check(L.crt_read_aov(sc._h, cr.AOV_HIT | cr.AOV_NORMAL, ptr, W * H * 16))]
    for call in calls:
        refused(call)
    with pytest.raises(ValueError):
        sc.read_aov(3)
    sc.set_option("accel", 1)                                  # the BVH2 walk has another tie rule
    refused(lambda: sc.render_aov(*RVS[1]))
    sc.set_option("accel", 0)
    assert not buf.any()
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(words(after[n]), words(before[n])), n
    assert np.array_equal(sc.read_sum().view(np.uint32), sum_before.view(np.uint32))
    sc.set_devices([0, 0])                                     # two logical devices behind the handle (the call itself restarts the sum)
    sc.render_frame(*RVS[0])
    sum_two = sc.read_sum()
    refused(lambda: sc.render_aov(*RVS[1]))
    assert np.array_equal(sc.read_sum().view(np.uint32), sum_two.view(np.uint32))
    sc.set_devices([0])
    after = read_all(cr, sc)
    for n in CHANNELS:
        assert np.array_equal(words(after[n]), words(before[n])), n
    # the device pointers hold the bytes read_aov returns
    for n in CHANNELS:
        p = sc.aov_device(bit_of(cr, n))
        assert p and np.array_equal(device_bytes_at(p, W * H * 16), np.ascontiguousarray(before[n]).view(np.uint8).reshape(-1)), n
    sc.close()                                                 # destroy with the buffers allocated
    # a fresh scene that never rendered a channel refuses the reads
    sc = flat_scene(cr, mesh, cam, "sbvh", W, H)
    refused(lambda: sc.read_aov(cr.AOV_HIT))
    refused(lambda: sc.aov_device(cr.AOV_HIT))
    sc.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["flat", "instanced"])
def test_g8_ten_calls_hold_the_memory_of_the_first(cr, cornell, textured, kind):
    import torch
    mesh, parts = flat_variants(cr, cornell, textured)["textured"]
    cam = cornell[1]
    W, H = SIZES[1]
    if kind == "flat":
        sc, inst = flat_scene(cr, mesh, cam, "sbvh", W, H), None
    else:
        inst, sc, _ = identity_scene(cr, mesh, parts, "sah", W, H)
        sc.update(cam)
    used = []
    for k in range(10):
        sc.render_aov(*RVS[k % 8])
        free, total = torch.cuda.mem_get_info()
        used.append(total - free)
    print("device bytes in use after each render_aov:", used)
    assert all(u == used[0] for u in used), used
    sc.close()
    if inst is not None:
        inst.close()


@pytest.mark.gpu
def test_g8_after_rebuild_vertices_the_buffers_show_the_new_positions(cr, ob, cornell, textured):
    mesh, _ = flat_variants(cr, cornell, textured)["tess8_mat"]
    cam = cornell[1]
    W, H = SIZES[1]
    rng = np.random.default_rng(5)
    moved = cr.Mesh((mesh.vertices + rng.uniform(-0.15, 0.15, mesh.vertices.shape)).astype(f32), mesh.normals, mesh.texcoords, mesh.triangles, mesh.materials,
                    mesh.lights, mesh.vertex_min)
    sc = flat_scene(cr, mesh, cam, "sah", W, H)
    sc.render_aov(*RVS[0])
    assert_channels(cr, read_all(cr, sc), flat_reference(cr, ob, "tess8_mat", "sah", mesh, flat_data(cr, mesh, cam, "sah"), cam, W, H, RVS[0], 1), "built")
    sc.rebuild_vertices(moved.vertices)
    sc.render_aov(*RVS[0])
    ref = flat_reference(cr, ob, "tess8_mat moved", "sah", moved, flat_data(cr, moved, cam, "sah"), cam, W, H, RVS[0], 1)
    got = read_all(cr, sc)
    assert_channels(cr, got, ref, "rebuilt")
    assert (words(got["HIT"]) != words(_FLAT[("tess8_mat", "sah", W, H, RVS[0], 1)]["HIT"])).any()
    sc.close()
