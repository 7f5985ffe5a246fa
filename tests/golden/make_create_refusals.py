"""Records tests/golden/create_refusals.json: what every case of tests/create_refusals.py gets from the library the binding loads (CRT_LIB
points it at another build, e.g. the commit before a change to scene creation).  Run on a GPU machine:

    python tests/golden/make_create_refusals.py [OUT.json]

A refusal is a return code and a text: two recordings of one library are identical.
DATA produced by running the library, not program text.
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import numpy as np
    import caitlynrenderer_amd as cr
    from conftest import _Cam
    import create_refusals as refusals
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "create_refusals.json")
    with open(os.path.join(HERE, "cornell_box.json")) as f:
        j = json.load(f)
    mesh = cr.Mesh(np.array(j["vertices"], np.float32), np.array(j["normals"], np.float32), np.zeros((0, 2), np.float32),
                   np.array(j["triangles"], np.int32), np.array(j["materials"], np.float32),
                   np.array(j["lights"], np.float32), np.array(j["vertex_min"], np.float32))
    data = cr.SceneData.build(mesh, _Cam(cr, j["camera"]))
    flat = refusals.observe_null_arguments(cr, mesh, data)
    for case in list(refusals.FLAT_HOST_CHECKS) + list(refusals.FLAT_DEVICE_CHECKS):
        flat[case] = refusals.observe_flat(cr, mesh, data, case)
        print(case, flat[case])
    handle = refusals.make_handle(cr, mesh)
    instanced = {}
    for case in refusals.INSTANCED_CHECKS:
        instanced[case] = refusals.observe_instanced(cr, mesh, handle, case)
        print(case, instanced[case])
    handle.close()
    with open(out, "w") as f:
        json.dump({"flat": flat, "instanced": instanced}, f, indent=1, sort_keys=True)
    print("wrote", out, len(flat), "+", len(instanced), "records")


if __name__ == "__main__":
    main()
