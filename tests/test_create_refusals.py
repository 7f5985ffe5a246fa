"""What the three scene creators refuse, held to a recording (tests/golden/create_refusals.json, made by
tests/golden/make_create_refusals.py with the library as it was before scene creation moved to crt_create.cpp): for every single-fault
descriptor of tests/create_refusals.py the return code, the text crt_last_error() gives and that *out came back NULL.  The flat-scene
checks that come before the library asks for a device run anywhere; the rest need the GPU."""
import json
import os

import pytest

import create_refusals as refusals

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "create_refusals.json")) as _f:
    RECORDED = json.load(_f)


def test_the_recording_covers_every_case():
    cases = ["null_out", "null_desc"] + list(refusals.FLAT_HOST_CHECKS) + list(refusals.FLAT_DEVICE_CHECKS)
    assert sorted(RECORDED["flat"]) == sorted(cases)
    assert sorted(RECORDED["instanced"]) == sorted(refusals.INSTANCED_CHECKS)
    for rec in list(RECORDED["flat"].values()) + list(RECORDED["instanced"].values()):      # every one of them a refusal with a text
        assert rec["rc"] < 0 and rec["error"] and rec["out_null"] in (True, None)


def test_null_arguments_are_refused_as_recorded(cr, cornell, cornell_data):
    got = refusals.observe_null_arguments(cr, cornell[0], cornell_data)
    print(got)
    assert got == {k: RECORDED["flat"][k] for k in ("null_out", "null_desc")}


@pytest.mark.parametrize("case", list(refusals.FLAT_HOST_CHECKS))
def test_flat_host_check_refuses_as_recorded(cr, cornell, cornell_data, case):
    got = refusals.observe_flat(cr, cornell[0], cornell_data, case)
    print(case, got)
    assert got == RECORDED["flat"][case]


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(refusals.FLAT_DEVICE_CHECKS))
def test_flat_device_check_refuses_as_recorded(cr, cornell, cornell_data, case):
    got = refusals.observe_flat(cr, cornell[0], cornell_data, case)
    print(case, got)
    assert got == RECORDED["flat"][case]


@pytest.fixture(scope="module")
def handle(cr, cornell):
    h = refusals.make_handle(cr, cornell[0])
    yield h
    h.close()


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(refusals.INSTANCED_CHECKS))
def test_instanced_creator_refuses_as_recorded(cr, cornell, handle, case):
    got = refusals.observe_instanced(cr, cornell[0], handle, case)
    print(case, got)
    assert got == RECORDED["instanced"][case]


@pytest.mark.gpu
def test_the_unedited_descriptors_are_accepted(cr, cornell, cornell_data, handle):
    """the cases are single faults: without its edit every base descriptor makes a scene (and a refused create has bound nothing to the handle)"""
    import ctypes as C
    from caitlynrenderer_amd._lib import check, lib
    mesh = cornell[0]
    textured = lambda f: f.with_textures()
    for data, edit in ((cornell_data, None), (None, None), (cornell_data, textured), (None, textured)):
        f = refusals.Flat(cr, mesh, data)
        if edit:
            edit(f)
        d, out = f.desc(), C.c_void_p()
        check(lib().crt_scene_create(C.byref(d), C.byref(out)))
        check(lib().crt_scene_destroy(out))
    for lit, edit in ((False, None), (True, None), (False, textured)):
        i = refusals.Instanced(mesh)
        if edit:
            edit(i)
        d, ml, keep = i.desc(handle._h)
        out = C.c_void_p()
        check(lib().crt_scene_create_instanced_lit(C.byref(d), ml, C.byref(out)) if lit else lib().crt_scene_create_instanced(C.byref(d), C.byref(out)))
        check(lib().crt_scene_destroy(out))
