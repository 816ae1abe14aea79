"""The deferred pack on the device (lc_field_pack_deferred; Engine.prepare_field): a float32 order-1 field longer than the first
launch of a fused advect call reaches has its first 33 levels packed at once and the rest inside the launches of the advect
call that follows, in pack workgroups among the advecting ones -- or, for every other use, by the stand-alone kernel first.
Positions and images are those of an engine created under ``LCS_DEFER_PACK=0``, bit for bit.

A 48 x 96-node float32 field, 512 x 512 seeds with two seeds per lane forced: the smallest grid that runs in level chunks
(``lcplan::CHUNK_FROM_SEEDS``), 512 advect workgroups + 8 pole workgroups, a grading zone of 96 positions.  nt = 72: three
graded launches, the first of which stays inside the packed levels (eligible; it carries levels 33 .. 71).  nt = 41: two
launches, the first of which reaches level 40 (the last boundary moves outwards): the call completes the pack first."""
import numpy as np
import pytest
import torch

from lagrangiancoherence_amd import flows

pytestmark = pytest.mark.gpu

DT, K = -1800.0, 4
FIRST = 33           # levels of lin the deferred entry packs at once (Engine.DEFER_FIRST_LEVELS + 1)
BOUNDARIES = {"cyclic": dict(cyclic_xboundary=True), "pointwise": dict(cyclic_xboundary=False, noncyclic_clamp="pointwise")}


@pytest.fixture(scope="module")
def setup():
    import os
    from lagrangiancoherence_amd.engine import Engine
    u, v, lat, lon = flows.era5_like(nt=72, ny=48, nx=96)
    slat, slon = flows.seed_grid(512, 512, lat, lon)
    was = os.environ.pop("LCS_DEFER_PACK", None)
    try:
        os.environ["LCS_DEFER_PACK"] = "0"           # (read once, when a context is created)
        ref = Engine(0)
        del os.environ["LCS_DEFER_PACK"]
        eng = Engine(0)
    finally:
        os.environ.pop("LCS_DEFER_PACK", None)
        if was is not None:
            os.environ["LCS_DEFER_PACK"] = was
    for e in (ref, eng):
        e.set_lds_tiles(1)        # the two-seed kernel whatever the size
    f32 = np.dtype(np.float32)
    S = dict(ref=ref, eng=eng, u=eng.to_device(u, f32), v=eng.to_device(v, f32), lat=lat, lon=lon, slat=eng.to_device(slat, f32),
             slon=eng.to_device(slon, f32), cache={})
    yield S
    eng.close()
    ref.close()


def field_of(S, e, nt):
    return e.prepare_field(S["u"][:nt], S["v"][:nt], S["lat"], S["lon"], 1)


def pending(e):
    return e.lib.lc_ctx_pack_pending(e.ctx)


def reference(S, nt, name, **kw):
    """The switched-off engine's field and positions for this call, computed once."""
    key = (nt, name, tuple(sorted(kw.items())))
    if key not in S["cache"]:
        ref = S["ref"]
        f = field_of(S, ref, nt)
        assert pending(ref) == 0 and f.pending is None
        S["cache"][key] = (f, ref.advect(f, S["slat"], S["slon"], DT, K, 1, **BOUNDARIES[name], **kw), ref.last_advect_launches())
    return S["cache"][key]


def same_images(f, g):
    return torch.equal(f.lin, g.lin) and torch.equal(f.ext, g.ext)


def check_call(S, nt, name, launches):
    eng = S["eng"]
    f0, (x0, y0), n0 = reference(S, nt, name)
    f = field_of(S, eng, nt)
    assert pending(eng) == FIRST and f.pending is not None
    x, y = eng.advect(f, S["slat"], S["slon"], DT, K, 1, **BOUNDARIES[name])
    if eng.last_advect_launches() != launches or n0 != launches:
        pytest.skip(f"the plan differs: {eng.last_advect_launches()} launches (reference {n0}), {launches} expected")
    assert eng.last_advect_kernel() == "advect_lds2_kernel<4, %s, 0>" % ("true" if name == "cyclic" else "false")
    assert eng.last_pack_kernel() == "pack_fused_kernel"
    assert pending(eng) == 0           # carried by the launches, or completed before them
    assert eng._pending is None and f.pending is None
    assert torch.equal(x, x0) and torch.equal(y, y0)
    assert same_images(f, f0)


@pytest.mark.parametrize("name", list(BOUNDARIES))
@pytest.mark.parametrize("nt, launches", [(72, 3), (41, 2)], ids=["nt72", "nt41"])
def test_positions_and_images_equal_the_switched_off_engine(setup, nt, launches, name):
    check_call(setup, nt, name, launches)


@pytest.mark.parametrize("nt, launches", [(72, 3), (41, 2)], ids=["nt72", "nt41"])
def test_uniform_chunks_of_32(setup, nt, launches):
    S = setup
    try:
        for e in (S["ref"], S["eng"]):
            e.set_level_chunk(32)
        S["cache"].pop((nt, "cyclic", ()), None)
        check_call(S, nt, "cyclic", launches)
    finally:
        S["cache"].pop((nt, "cyclic", ()), None)
        for e in (S["ref"], S["eng"]):
            e.set_level_chunk(-1)


def test_images_read_before_any_advect_are_whole(setup):
    S, eng = setup, setup["eng"]
    f0 = reference(S, 72, "cyclic")[0]
    f = field_of(S, eng, 72)
    assert pending(eng) == FIRST
    lin = f.lin                        # reading either attribute completes the pack
    assert pending(eng) == 0 and f.pending is None
    assert torch.equal(lin, f0.lin) and torch.equal(f.ext, f0.ext)
    g = field_of(S, eng, 72)
    assert pending(eng) == FIRST and torch.equal(g.ext, f0.ext) and pending(eng) == 0 and torch.equal(g.lin, f0.lin)


def test_a_first_call_that_cannot_carry_the_pack(setup):
    S, eng, ref = setup, setup["eng"], setup["ref"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    a = (S["slat"], S["slon"], DT)
    # SETTLS_order = 0
    f = field_of(S, eng, 72)
    xk, yk = eng.advect(f, *a, 0, 1, True)
    assert pending(eng) == 0
    rk = ref.advect(f0, *a, 0, 1, True)
    assert torch.equal(xk, rk[0]) and torch.equal(yk, rk[1])
    x, y = eng.advect(f, *a, K, 1, True)
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)
    # trajectories (40 levels)
    f = field_of(S, eng, 72)
    out = eng.advect(f, *a, K, 1, True, nsteps=40, return_traj=True)
    assert pending(eng) == 0
    want = ref.advect(f0, *a, K, 1, True, nsteps=40, return_traj=True)
    assert all(torch.equal(p, q) for p, q in zip(out, want))
    x, y = eng.advect(f, *a, K, 1, True)
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)
    # an order-1 sample of a level the first pack did not reach
    f = field_of(S, eng, 72)
    su, sv = eng.sample(f, x0, y0, level=60, interp_order=1)
    assert pending(eng) == 0
    wu, wv = ref.sample(f0, x0, y0, level=60, interp_order=1)
    assert torch.equal(su, wu) and torch.equal(sv, wv)
    x, y = eng.advect(f, *a, K, 1, True)
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)


def test_an_order_1_tracer_sample_completes_the_pack(setup):
    """``lc_tracer_sample`` reads other images altogether (the tracer's); it completes the context's pending pack like every
    entry point that takes image pointers, and the K = 4 call that follows finds whole images."""
    S, eng, ref = setup, setup["eng"], setup["ref"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    a = (S["slat"], S["slon"], DT)
    lat, lon = S["lat"], S["lon"]
    tr, tr0 = eng.prepare_tracer(S["v"], None, lat, lon, 1), ref.prepare_tracer(S["v"], None, lat, lon, 1)
    _, _, tx, ty = ref.advect(f0, *a, K, 1, True, nsteps=6, return_traj=True)
    want = ref.sample_tracer(tr0, tx, ty, level0=40, interp_order=1)
    f = field_of(S, eng, 72)
    assert pending(eng) == FIRST
    got = eng.sample_tracer(tr, tx, ty, level0=40, interp_order=1)
    assert pending(eng) == 0 and f.pending is not None          # completed by the C entry point, not through the attributes
    assert torch.equal(got[0][0], want[0][0])
    x, y = eng.advect(f, *a, K, 1, True)
    assert f.pending is None and torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)


def test_planes_written_while_the_pack_is_pending_are_refused(setup):
    """The levels not packed yet are read from the caller's planes later: writing them in place meanwhile is refused, as for
    every field that borrows its planes."""
    S, eng = setup, setup["eng"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    f = field_of(S, eng, 72)
    S["u"].add_(0.0)                    # (the same values: only the version counter moves)
    with pytest.raises(RuntimeError, match="modified in place"):
        eng.advect(f, S["slat"], S["slon"], DT, K, 1, True)
    with pytest.raises(RuntimeError, match="modified in place"):
        f.lin
    with pytest.raises(RuntimeError, match="modified in place"):
        field_of(S, eng, 72)
    assert pending(eng) == FIRST and f.pending is not None      # still pending: nothing was packed from the written planes
    eng.lib.lc_ctx_flush_pack(eng.ctx)                            # (the values are the same here: complete it by hand)
    assert torch.equal(f.lin, f0.lin) and torch.equal(f.ext, f0.ext)
    # once the pack is complete the planes are the caller's again (a float32 order-1 field never read them after its pack)
    g = field_of(S, eng, 72)
    x, y = eng.advect(g, S["slat"], S["slon"], DT, K, 1, True)
    S["u"].add_(0.0)
    x, y = eng.advect(g, S["slat"], S["slon"], DT, K, 1, True)
    assert torch.equal(x, x0) and torch.equal(y, y0)


def test_planes_written_are_refused_whatever_would_complete_the_pack(setup):
    """Most library calls complete a pending pack on their own, from the planes as they are then: the stamps are looked at
    before every call the engine makes, so none of them packs the later levels from planes written meanwhile."""
    from lagrangiancoherence_amd.engine import Engine
    S, eng, ref = setup, setup["eng"], setup["ref"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    a = (S["slat"], S["slon"], DT)
    other = field_of(S, eng, 72)
    assert other.lin is not None and pending(eng) == 0          # a whole field of the same engine
    tr = eng.prepare_tracer(S["v"], None, S["lat"], S["lon"], 1)
    _, _, tx, ty = ref.advect(f0, *a, K, 1, True, nsteps=3, return_traj=True)
    f = field_of(S, eng, 72)
    S["u"].add_(0.0)                    # (the same values: only the version counter moves)
    side = torch.cuda.Stream(eng.device)
    side.wait_stream(torch.cuda.current_stream(eng.device))
    with torch.cuda.stream(side):       # the change of stream would complete the pack before the call's own check
        with pytest.raises(RuntimeError, match="modified in place"):
            eng.advect(f, *a, K, 1, True)
    assert pending(eng) == FIRST
    for call in (lambda: eng.advect(other, *a, K, 1, True), lambda: eng.sample(other, x0, y0, level=3, interp_order=1),
                 lambda: eng.sample_tracer(tr, tx, ty, level0=40, interp_order=1), lambda: field_of(S, eng, 41)):
        with pytest.raises(RuntimeError, match="modified in place"):
            call()
        assert pending(eng) == FIRST and f.pending is not None   # still pending: nothing was packed from the written planes
    eng.lib.lc_ctx_flush_pack(eng.ctx)                            # (the values are the same here: complete it by hand)
    x, y = eng.advect(f, *a, K, 1, True)
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)
    # an engine that is closed with such a pack cannot refuse: the field is refused wherever it is used next
    e2 = Engine(0)
    g = e2.prepare_field(S["u"][:72], S["v"][:72], S["lat"], S["lon"], 1)
    assert pending(e2) == FIRST
    S["v"].add_(0.0)
    e2.close()
    with pytest.raises(RuntimeError, match="modified in place"):
        g.lin
    with pytest.raises(RuntimeError, match="modified in place"):
        ref.advect(g, *a, K, 1, True)
    # closed with the planes untouched, the field is whole
    e3 = Engine(0)
    h = e3.prepare_field(S["u"][:72], S["v"][:72], S["lat"], S["lon"], 1)
    e3.close()
    assert same_images(h, f0)


def test_advect_on_a_side_stream_waits_for_the_rest_of_the_pack(setup):
    """The usual idiom -- ``side.wait_stream(cur)``, then the advect under ``torch.cuda.stream(side)`` -- recorded its wait
    before the context completed the pack on ``cur``: the context makes the side stream wait for that kernel itself."""
    S, eng = setup, setup["eng"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    cur, side = torch.cuda.current_stream(eng.device), torch.cuda.Stream(eng.device)
    f = field_of(S, eng, 72)
    side.wait_stream(cur)
    with torch.cuda.stream(side):
        x, y = eng.advect(f, S["slat"], S["slon"], DT, K, 1, True)
    cur.wait_stream(side)
    assert pending(eng) == 0 and torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)


def test_a_field_advected_through_another_engine_is_completed_first(setup):
    S, eng, ref = setup, setup["eng"], setup["ref"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    f = field_of(S, eng, 72)
    assert pending(eng) == FIRST
    x, y = ref.advect(f, S["slat"], S["slon"], DT, K, 1, True)       # ref's context has nothing pending: the engine completes eng's
    assert pending(eng) == 0 and f.pending is None and eng._pending is None
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(f, f0)


def test_two_fields_prepared_back_to_back(setup):
    S, eng = setup, setup["eng"]
    f0, (x0, y0), _ = reference(S, 72, "cyclic")
    f41, (x41, y41), _ = reference(S, 41, "cyclic")
    a = field_of(S, eng, 72)
    b = field_of(S, eng, 41)           # one pending pack per context: a's is completed here
    assert pending(eng) == FIRST
    x, y = eng.advect(a, S["slat"], S["slon"], DT, K, 1, True)
    assert pending(eng) == 0           # (other images: b's pack is completed before a's call)
    assert torch.equal(x, x0) and torch.equal(y, y0) and same_images(a, f0)
    x, y = eng.advect(b, S["slat"], S["slon"], DT, K, 1, True)
    assert torch.equal(x, x41) and torch.equal(y, y41) and same_images(b, f41)


@pytest.mark.parametrize("rows", [(128, 384), (0, 256), (256, 512)], ids=["inner block with halo", "south pole rows", "north pole rows"])
def test_row_blocks(setup, rows):
    S, eng, ref = setup, setup["eng"], setup["ref"]
    lo, hi = rows
    f0 = reference(S, 72, "cyclic")[0]
    kw = dict(row0=lo, ny_global=512, halo=(2, 2) if lo > 0 and hi < 512 else None)
    try:
        for e in (ref, eng):
            e.set_level_chunk(16)      # (a block of 256 rows is one launch by size: chunks of 16 levels, so that its launches carry the pack)
        want = ref.advect(f0, S["slat"][lo:hi], S["slon"], DT, K, 1, True, **kw)
        f = field_of(S, eng, 72)
        assert pending(eng) == FIRST
        got = eng.advect(f, S["slat"][lo:hi], S["slon"], DT, K, 1, True, **kw)
        assert pending(eng) == 0 and eng.last_advect_launches() == ref.last_advect_launches() == 5
    finally:
        for e in (ref, eng):
            e.set_level_chunk(-1)
    n = 2 if kw["halo"] else 0
    for p, q in zip(got, want):
        assert torch.equal(p[n:n + hi - lo], q[n:n + hi - lo])
    assert same_images(f, f0)
