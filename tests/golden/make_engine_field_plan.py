"""Record ``tests/golden/engine_field_plan.json``: what ``Engine.prepare_field`` and ``Engine._advect_args`` decided at the
commit BEFORE the engine got its field plan and its one argument fill (``tests/engine_plan.py`` holds the cases).

    git checkout <parent> -- lagrangiancoherence_amd/engine.py && python tests/golden/make_engine_field_plan.py <parent>

The file is the parent's behaviour and is not regenerated from later code: ``call_args`` below is the parent's positional
``_advect_args``, which no longer exists.  Runs on the CPU in seconds; two runs give the same bytes."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from tests import engine_plan as EP  # noqa: E402


def call_args(eng, field, interp_order, xmode, bufs, scal):
    ny, nx = EP.SEEDS
    g = bufs.get
    return eng._advect_args(field, interp_order, bufs["seed_lat"], ny, bufs["seed_lon"], nx, scal.get("row0", 0),
                            scal.get("ny_global", ny), g("start_x"), g("start_y"), scal["timestep"], scal["K"], xmode,
                            scal.get("t0", 0), scal["nsteps"], scal.get("n_members", 1), scal.get("t0_stride", 0),
                            bufs["out_x"], bufs["out_y"], g("traj_x"), g("traj_y"))


if __name__ == "__main__":
    doc = {"recorded_at": sys.argv[1], "grid": [EP.NY_F, EP.NX_F], **EP.record(call_args)}
    with open(os.path.join(HERE, "engine_field_plan.json"), "w") as f:
        f.write(EP.dumps(doc))
    for k in ("prepare_field", "advect_args", "stale_wind"):
        print(k, len(doc[k]["cases"]), "cases,", len(doc[k]["outcomes"]), "distinct outcomes")
