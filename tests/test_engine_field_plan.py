"""The engine's field plan and call source against the decisions of the engine before it had them
(tests/golden/engine_field_plan.json, recorded by tests/golden/make_engine_field_plan.py at the commit the file names):
every ``prepare_field`` option combination, every ``_advect_args`` source, and the stale-wind guard on every path that builds
a call's arguments -- replayed on the CPU through tests/engine_plan.py's stand-in library and compared exactly."""
import json
import os

import numpy as np
import pytest

from lagrangiancoherence_amd import engine as E
from tests import engine_plan as EP

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "engine_field_plan.json")) as _f:
    GOLDEN = json.load(_f)


def call_args(eng, field, interp_order, xmode, bufs, scal):
    """``Engine._advect_args`` with the geometry by keyword; what ``scal`` leaves out stays at its default."""
    pair = lambda a, b: (bufs[a], bufs[b]) if a in bufs else None
    scal = dict(scal)
    return eng._advect_args(field, interp_order, bufs["seed_lat"], EP.SEEDS[0], bufs["seed_lon"], EP.SEEDS[1], scal.pop("timestep"),
                            scal.pop("K"), xmode, start=pair("start_x", "start_y"), out=pair("out_x", "out_y"),
                            traj=pair("traj_x", "traj_y"), **scal)


def _mismatches(table, cases, outcome):
    want, index = GOLDEN[table]["outcomes"], GOLDEN[table]["cases"]
    assert len(index) == len(cases)
    # (through json, as the golden file went: tuples and lists, numpy and python scalars compare as what was written)
    return [(c, got, want[i]) for c, i in zip(cases, index) for got in [json.loads(json.dumps(outcome(*c)))] if got != want[i]]


def test_the_golden_file_is_the_parents_and_covers_every_case():
    assert len(GOLDEN["recorded_at"]) == 40 and GOLDEN["grid"] == [EP.NY_F, EP.NX_F]
    pf = GOLDEN["prepare_field"]
    assert len(pf["cases"]) == 3 * 5 * 3 * 27 == 1215 and len(pf["outcomes"]) == 109
    assert sum("error" in pf["outcomes"][i] for i in pf["cases"]) == 27
    assert len(GOLDEN["advect_args"]["cases"]) == len(EP.args_cases()) == 270
    # every borrowed-plane field refuses a stale wind on every path
    assert len(GOLDEN["stale_wind"]["cases"]) == len(EP.stale_cases()) and len(GOLDEN["stale_wind"]["outcomes"]) == 1
    assert GOLDEN["stale_wind"]["outcomes"][0].startswith("the wind tensors given to prepare_field were modified in place")


def test_prepare_field_decides_what_the_parent_decided():
    eng = EP.stub_engine()
    bad = _mismatches("prepare_field", EP.field_cases(), lambda *c: EP.field_outcome(eng, *c))
    assert not bad, (len(bad), bad[:3])


def test_advect_args_are_what_the_parent_filled():
    eng = EP.stub_engine()
    bad = _mismatches("advect_args", EP.args_cases(), lambda *c: EP.args_outcome(eng, call_args, *c))
    assert not bad, (len(bad), bad[:3])


def test_a_stale_wind_is_refused_on_every_path_that_builds_arguments():
    eng = EP.stub_engine()
    bad = _mismatches("stale_wind", EP.stale_cases(), lambda *c: EP.stale_outcome(eng, call_args, *c))
    assert not bad, (len(bad), bad[:3])


def _plan_outcome(kind, order, nt, fuse_levels, lin_image, ext_image, plan_fn=None):
    """What the plan alone says ``prepare_field`` will do, in the golden file's terms."""
    dtype = np.dtype(EP.KINDS[kind][1])
    p = (plan_fn or E.field_plan)(dtype, kind == "wind_f32", order, nt, fuse_levels, lin_image, ext_image,
                                  E.Engine.EXT_IMAGE_F64, E.Engine.EXT_IMAGE_F64_O3)
    if p.refusal:
        return {"error": p.refusal}
    stamps = {("u", "v"): ["planes_version"], ("u32", "v32"): ["planes32_version"], (): []}[p.planes]
    has = set(p.images) | set(p.planes) | set(stamps)
    return {"packs": [[code, nt, o, image is not None, bool(ext)] for code, o, image, ext in p.packs],
            "present": [a for a in EP.FIELD_ATTRS if a in has], "wind_f32": p.wind_f32, "order": p.order,
            "fuse_raw": p.fuse_raw, "dtype": dtype.name}


def test_the_plan_alone_says_what_prepare_field_did():
    bad = _mismatches("prepare_field", EP.field_cases(), _plan_outcome)
    assert not bad, (len(bad), bad[:3])
    for kind, order, nt, *options in EP.field_cases():       # ... and is consistent in itself
        p = E.field_plan(EP.KINDS[kind][1], kind == "wind_f32", order, nt, *options, E.Engine.EXT_IMAGE_F64, E.Engine.EXT_IMAGE_F64_O3)
        assert all(image is None or image in p.images for _, _, image, _ in p.packs) and all("ext" in p.images for *_, e in p.packs if e)
        assert all(0 < levels <= nt for levels in p.images.values()) and p.images.get("ext", nt - 1) == nt - 1
        assert p.upload == (np.float32 if p.planes == ("u32", "v32") else np.dtype(EP.KINDS[kind][1]))


@pytest.mark.parametrize("decision", ["fuse_raw", "planes", "packs", "wind_f32", "refusal"])
def test_one_flipped_decision_in_the_plan_is_caught(monkeypatch, decision):
    """The replay is not vacuous: a plan that differs in one decision fails it, through ``prepare_field`` and alone."""
    real = E.field_plan

    def flipped(*a):
        p = real(*a)
        return p._replace(**{"fuse_raw": dict(fuse_raw=not p.fuse_raw), "planes": dict(planes=("u", "v") if not p.planes else ()),
                             "packs": dict(packs=p.packs[1:]),
                             "wind_f32": dict(wind_f32=not p.wind_f32), "refusal": dict(refusal=None)}[decision])
    monkeypatch.setattr(E, "field_plan", flipped)
    eng = EP.stub_engine()
    assert _mismatches("prepare_field", EP.field_cases(), lambda *c: EP.field_outcome(eng, *c))
    assert _mismatches("prepare_field", EP.field_cases(), lambda *c: _plan_outcome(*c, plan_fn=flipped))


def test_one_flipped_decision_in_the_call_source_is_caught(monkeypatch):
    real = E.call_source
    monkeypatch.setattr(E, "call_source", lambda f, o, x: real(f, o, x)._replace(fuse_levels_raw=1 - real(f, o, x).fuse_levels_raw))
    eng = EP.stub_engine()
    assert _mismatches("advect_args", EP.args_cases(), lambda *c: EP.args_outcome(eng, call_args, *c))
    # ... and a source that no longer asks for the float64 planes leaves u_raw / v_raw empty
    monkeypatch.setattr(E, "call_source", lambda f, o, x: real(f, o, x)._replace(planes64=False))
    assert _mismatches("advect_args", EP.args_cases(), lambda *c: EP.args_outcome(eng, call_args, *c))
