"""Records tests/golden/frame_forms.json: what every configuration of tests/frame_forms.py produces on the MI355X with the library the
binding loads (CRT_LIB points it at another build, e.g. the commit before a change to the frame dispatch).  Run on a GPU machine:

    python tests/golden/make_frame_forms.py [OUT.json]

The frames are bit-reproducible, so two recordings are expected to be identical: record twice and compare.  With a second argument, a
recording made earlier, a configuration whose hash differs between the two is written without its hash and named on stdout.
DATA produced by running the library, not program text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scenes():
    import numpy as np
    import caitlynrenderer_amd as cr
    from caitlynrenderer_amd.meshgen import tessellated_cornell
    from conftest import _Cam
    import frame_forms as ff
    with open(os.path.join(HERE, "cornell_box.json")) as f:
        j = json.load(f)
    mesh = cr.Mesh(np.array(j["vertices"], np.float32), np.array(j["normals"], np.float32), np.zeros((0, 2), np.float32),
                   np.array(j["triangles"], np.int32), np.array(j["materials"], np.float32),
                   np.array(j["lights"], np.float32), np.array(j["vertex_min"], np.float32))
    cam = _Cam(cr, j["camera"])
    candidates = []
    for n in (8, 40):                      # conftest's tess8 and tess40
        m = tessellated_cornell(mesh, n)
        candidates.append((f"tess{n}", m, cr.SceneData.build(m, cam)))
    return ff.Scenes(cr, (mesh, cam), cr.SceneData.build(mesh, cam), candidates)


def main():
    import frame_forms as ff
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "frame_forms.json")
    earlier = json.load(open(sys.argv[2]))["records"] if len(sys.argv) > 2 else None
    sc = scenes()
    records = {}
    for cid, cfg in ff.configurations():
        rec = ff.observe(sc, cfg)
        if earlier is not None and earlier[cid] != rec:
            print("differs between two recordings:", cid, earlier[cid], rec)
            if {k: v for k, v in earlier[cid].items() if k != "sha256"} == {k: v for k, v in rec.items() if k != "sha256"}:
                rec.pop("sha256")
        records[cid] = rec
        print(cid, rec)
    json.dump({"frame": [ff.W, ff.H], "big": sc.big_name, "records": records}, open(out, "w"), indent=1, sort_keys=True)
    print("wrote", out, len(records), "records; big =", sc.big_name)


if __name__ == "__main__":
    main()
