"""Helpers of the finite-size-exponent tests (tests/test_fsle.py, tests/test_fsle_gpu.py): the definition of include/lcs_hip.h
("finite-size Lyapunov exponents") restated in numpy for any arithmetic dtype -- float32 / float64 as csrc/fsle.hip runs it,
``np.longdouble`` as the judge, which is run on the very float32 / float64 positions the kernel is given --, the margins the
tests leave cells out by, and an analytic trajectory generator.  No expected value here comes from the engine.

Two restatements: :func:`definition` is the definition read literally (every pair's first upcrossing, then the minimum over a
cell's pairs); :func:`update` is the streaming form (one block of levels, tau / fsle carried), which walks the levels in order and
closes a cell at the first level where a pair of it upcrosses.  tests/test_fsle.py holds them equal.

k = pi / 180 with the float64 pi in every dtype (the kernels' constant; the judge's 1e-16 is far below every bound here)."""
import numpy as np

R_EARTH = 6371000.0
PAIRS = ("E", "W", "N", "S")


def separation(x1, y1, x2, y2, T, radius=R_EARTH):
    """Great-circle distance in half-angle form, in T; a NaN position gives NaN."""
    k = T(np.pi) / T(180)
    with np.errstate(invalid="ignore"):
        sp = np.sin(T(0.5) * (k * (y2 - y1)))
        sl = np.sin(T(0.5) * (k * (x2 - x1)))
        h = sp * sp + (np.cos(k * y1) * np.cos(k * y2)) * (sl * sl)
        return (T(2) * T(radius)) * np.arcsin(np.minimum(T(1), np.sqrt(h)))


def cell_separations(x, y, T, cyclic, radius=R_EARTH):
    """Separations of every cell's four pairs: ``(..., 4, ny, nx)`` in T for positions ``(..., ny, nx)``, NaN where the pair does
    not exist.  Every pair is evaluated once and handed to both of its cells: the same numbers."""
    x, y = np.asarray(x).astype(T), np.asarray(y).astype(T)
    ny, nx = x.shape[-2:]
    out = np.full(x.shape[:-2] + (4, ny, nx), np.nan, dtype=T)
    if nx > 1 or cyclic:
        if cyclic:        # pair c joins column c and column (c + 1) % nx
            ew = separation(x, y, np.roll(x, -1, axis=-1), np.roll(y, -1, axis=-1), T, radius)
            out[..., 0, :, :] = ew
            out[..., 1, :, :] = np.roll(ew, 1, axis=-1)
        else:
            ew = separation(x[..., :-1], y[..., :-1], x[..., 1:], y[..., 1:], T, radius)
            out[..., 0, :, :-1] = ew
            out[..., 1, :, 1:] = ew
    if ny > 1:
        ns = separation(x[..., :-1, :], y[..., :-1, :], x[..., 1:, :], y[..., 1:, :], T, radius)
        out[..., 2, :-1, :] = ns
        out[..., 3, 1:, :] = ns
    return out


def seed_separations(seed_lat, seed_lon, T, cyclic, radius=R_EARTH):
    lat, lon = np.asarray(seed_lat).astype(T), np.asarray(seed_lon).astype(T)
    return cell_separations(np.broadcast_to(lon[None, :], (lat.size, lon.size)), np.broadcast_to(lat[:, None], (lat.size, lon.size)),
                            T, cyclic, radius)


def record_separations(traj_x, traj_y, seed_lat, seed_lon, T, cyclic, radius=R_EARTH):
    """``(n_levels, 4, ny, nx)``: the separations of a whole record (level0 == 0); entry 0 is formed from the seeds."""
    D = cell_separations(traj_x, traj_y, T, cyclic, radius)
    D[0] = seed_separations(seed_lat, seed_lon, T, cyclic, radius)
    return D


def _thresholds(thresholds, mode, d0, T):
    """``(n_thr, 4, ny, nx)`` thresholds in T and the eligibility of every pair for every threshold."""
    thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64)).astype(T)
    assert mode in ("ratio", "distance")
    with np.errstate(invalid="ignore"):
        Tq = thr[:, None, None, None] * d0[None] if mode == "ratio" else np.broadcast_to(thr[:, None, None, None], (thr.size,) + d0.shape).copy()
        elig = np.isfinite(d0)[None] & (d0[None] > 0) & (d0[None] < Tq)
    return thr, Tq, elig


def _pick(t, Tq, d0, thr, mode, T):
    """Cell outputs from the pairs' times ``t`` (n_thr, 4, ny, nx; NaN: none): the minimum, ties to the first pair."""
    key = np.where(np.isnan(t), np.inf, t)
    p = np.argmin(key, axis=1)                                  # first minimum: E, W, N, S
    tau = np.take_along_axis(t, p[:, None], axis=1)[:, 0]
    Tp = np.take_along_axis(Tq, p[:, None], axis=1)[:, 0]
    d0p = np.take_along_axis(np.broadcast_to(d0[None], Tq.shape), p[:, None], axis=1)[:, 0]
    with np.errstate(invalid="ignore", divide="ignore"):
        num = np.log(thr)[:, None, None] if mode == "ratio" else np.log(Tp / d0p)
        fsle = np.where(np.isnan(tau), T(np.nan), num / tau)
    return tau.astype(T), fsle.astype(T), np.where(np.isnan(tau), -1, p)


def definition(traj_x, traj_y, seed_lat, seed_lon, thresholds, mode, timestep, T, cyclic=False, radius=R_EARTH) -> dict:
    """The definition, literally, on a whole record in arithmetic T.  Returns ``tau``, ``fsle`` (n_thr, ny, nx), and what the
    tests judge by: ``pair`` (index into PAIRS of the pair that gave the minimum, -1: none), ``level`` (its crossing level j, 0:
    none), ``margin`` (the smallest |d_p(j) - T| / T over the cell's pairs and levels: level 0 of every pair, which decides its
    eligibility, and every later level of the eligible ones), ``before`` / ``after`` / ``thr`` (d_p*(j-1), d_p*(j) and T of the
    winning pair), ``pairs`` (per pair, ``(n_thr, 4, ny, nx)``: its time ``t``, crossing ``level``, ``before``, ``after``, ``thr``,
    the numerator ``num`` = ln(T / d0) and its own ``fsle``; NaN / 0 where it never upcrosses) and ``D`` (the separations)."""
    D = record_separations(traj_x, traj_y, seed_lat, seed_lon, T, cyclic, radius)
    L = D.shape[0]
    d0 = D[0]
    thr, Tq, elig = _thresholds(thresholds, mode, d0, T)
    dt = T(abs(float(timestep)))
    with np.errstate(invalid="ignore", divide="ignore"):
        up = elig[None] & (D[:-1, None] < Tq[None]) & (Tq[None] <= D[1:, None])          # (L-1, n_thr, 4, ny, nx): level j = index + 1
        any_up = up.any(axis=0)
        j = np.where(any_up, up.argmax(axis=0) + 1, 1)                                     # first upcrossing
        a = np.take_along_axis(np.broadcast_to(D[:, None], (L,) + Tq.shape), (j - 1)[None], axis=0)[0]
        b = np.take_along_axis(np.broadcast_to(D[:, None], (L,) + Tq.shape), j[None], axis=0)[0]
        t = np.where(any_up, ((j - 1).astype(T) + (Tq - a) / (b - a)) * dt, T(np.nan))
        tau, fsle, pair = _pick(t, Tq, d0, thr, mode, T)
        sel = np.maximum(pair, 0)[:, None]
        level = np.where(pair >= 0, np.take_along_axis(j, sel, axis=1)[:, 0], 0)
        rel = np.abs(D[:, None] - Tq[None]) / Tq[None]                                      # (L, n_thr, 4, ny, nx)
        counted = np.isfinite(rel) & np.concatenate([np.broadcast_to(np.isfinite(d0)[None, None], (1,) + elig.shape),
                                                     np.broadcast_to(elig[None], (L - 1,) + elig.shape)], axis=0)
        margin = np.where(counted, rel, np.inf).min(axis=(0, 2))
    pickp = lambda v: np.where(pair >= 0, np.take_along_axis(v, sel, axis=1)[:, 0], T(np.nan))
    with np.errstate(invalid="ignore", divide="ignore"):
        num = np.broadcast_to(np.log(thr)[:, None, None, None], Tq.shape) if mode == "ratio" else np.log(Tq / d0[None])
        pairs = dict(t=t, level=np.where(any_up, j, 0), before=np.where(any_up, a, T(np.nan)), after=np.where(any_up, b, T(np.nan)),
                     thr=Tq, num=num, fsle=np.where(any_up, num / t, T(np.nan)))
    return dict(tau=tau, fsle=fsle, pair=pair, level=level, margin=margin, before=pickp(a), after=pickp(b), thr=pickp(Tq),
                pairs=pairs, D=D)


def update(traj_x, traj_y, seed_lat, seed_lon, thresholds, mode, timestep, level0, T, tau=None, fsle=None, cyclic=False,
           radius=R_EARTH):
    """The streaming form on one block of levels, in arithmetic T: returns new ``(tau, fsle)``.  ``level0 == 0``: tau and fsle
    start as NaN and entry 0 is the seed grid."""
    D = cell_separations(traj_x, traj_y, T, cyclic, radius)
    d0 = seed_separations(seed_lat, seed_lon, T, cyclic, radius)
    if level0 == 0:
        D[0] = d0
    thr, Tq, elig = _thresholds(thresholds, mode, d0, T)
    shape = (thr.size,) + d0.shape[1:]
    tau = np.full(shape, np.nan, dtype=T) if level0 == 0 else np.array(tau, dtype=T)
    fsle = np.full(shape, np.nan, dtype=T) if level0 == 0 else np.array(fsle, dtype=T)
    dt = T(abs(float(timestep)))
    for j in range(1, D.shape[0]):
        with np.errstate(invalid="ignore", divide="ignore"):
            up = elig & (D[j - 1][None] < Tq) & (Tq <= D[j][None])
            t = np.where(up, (T(level0 + j - 1) + (Tq - D[j - 1][None]) / (D[j][None] - D[j - 1][None])) * dt, T(np.nan))
        tj, fj, _ = _pick(t, Tq, d0, thr, mode, T)
        take = np.isnan(tau) & ~np.isnan(tj)                    # a cell whose tau is finite is final
        tau[take], fsle[take] = tj[take], fj[take]
    return tau, fsle


def update_in_blocks(traj_x, traj_y, seed_lat, seed_lon, thresholds, mode, timestep, T, block, **kw):
    """:func:`update` over a whole record cut into blocks of ``block`` steps (entry 0 of a block: the last entry of the one before)."""
    L = np.shape(traj_x)[0]
    tau = fsle = None
    for lo in range(0, L - 1, block):
        hi = min(lo + block, L - 1)
        tau, fsle = update(traj_x[lo:hi + 1], traj_y[lo:hi + 1], seed_lat, seed_lon, thresholds, mode, timestep, lo, T, tau, fsle, **kw)
    return tau, fsle


# ------------------------------------------------------------------ what the tests leave out, and by how much they bound
def distance_error(traj_x, traj_y, seed_lat, seed_lon, T, cyclic, radius=R_EARTH) -> float:
    """The largest relative error of the numpy restatement's separations in T against longdouble, on these very positions."""
    D = record_separations(traj_x, traj_y, seed_lat, seed_lon, T, cyclic, radius).astype(np.longdouble)
    J = record_separations(traj_x, traj_y, seed_lat, seed_lon, np.longdouble, cyclic, radius)
    ok = np.isfinite(J) & (J > 0)
    return float(np.max(np.abs(D[ok] - J[ok]) / J[ok]))


def bounds(judge: dict, E: float, eps: float, timestep) -> dict:
    """What a computation whose separations are off by at most E relative (and whose other operations round by eps) may return,
    given the judge's record.  Per pair: with a = d(j-1), b = d(j) and T (a multiple of a separation in ratio mode) each off by
    E, the fraction f = (T - a) / (b - a) moves by at most (E (T + a) + f E (a + b)) / (b - a - E (a + b)) <= E (T + 2a + b) /
    (b - a - E (a + b)); the sum with j - 1, the product with |timestep| and the division round by at most 4 eps j.  That, in
    seconds, is the pair's bound ``t_bound`` -- inf where the denominator keeps less than half of b - a.  The cell's minimum
    can come from any pair whose interval [t - bound, t + bound] reaches below the winner's upper end (``relevant``), so the
    cell's ``tau_bound`` is the largest bound among those.  A pair's fsle = num / t is off by at most t_bound / (t - t_bound) +
    E / |num| (the numerator ln(T / d0) moves by E; exact in ratio mode but for rounding) + 4 eps, relative: ``fsle_bound``.
    ``left_out``: cells the comparison skips -- a separation within E of the threshold at some level (eligibility, the
    crossing level or the crossing itself may differ), or no finite bound."""
    P = judge["pairs"]
    a, b, Tq, t, num, f = (P[k].astype(np.float64) for k in ("before", "after", "thr", "t", "num", "fsle"))
    dt = abs(float(timestep))
    with np.errstate(invalid="ignore", divide="ignore"):
        den = (b - a) - E * (a + b)
        tb = np.where(den >= 0.5 * (b - a), (E * (Tq + 2 * a + b) / den + 4 * eps * P["level"]) * dt, np.inf)
        tb = np.where(np.isnan(t), np.inf, tb)
        tk = np.where(np.isnan(t), np.inf, t)
        win = np.maximum(judge["pair"], 0)[:, None]
        top = (np.take_along_axis(tk, win, axis=1) + np.take_along_axis(tb, win, axis=1))
        relevant = np.isfinite(tk) & (tk - np.where(np.isfinite(tb), tb, 0) <= top)
        tau_bound = np.where(relevant, tb, 0).max(axis=1)
        fb = np.abs(f) * (tb / (t - tb) + E / np.abs(num) + 4 * eps)
        fb = np.where(np.isfinite(tb) & (tb < t), fb, np.inf)
    crossed = judge["pair"] >= 0
    left = (judge["margin"] <= E) | (crossed & ~np.isfinite(tau_bound))
    return dict(t_bound=tb, relevant=relevant, tau_bound=tau_bound, fsle_bound=fb, left_out=left)


def check_against_judge(tau, fsle, judge: dict, B: dict, timestep) -> dict:
    """``tau``, ``fsle`` of the code under test against the judge, outside ``B['left_out']``: the NaN pattern is the judge's;
    tau lies in the crossing interval of a relevant pair and within the cell's bound of the judge's tau; fsle lies within a
    relevant pair's own bound of that pair's value (one pair is relevant in all but a few cells: then it is the judge's pair).
    Returns the figures (after asserting): the number of compared cells, of cells with more than one relevant pair, the largest
    relative tau and fsle errors and the largest relative tau bound."""
    tau, fsle = np.asarray(tau).astype(np.float64), np.asarray(fsle).astype(np.float64)
    keep = ~B["left_out"]
    jt, crossed = judge["tau"].astype(np.float64), judge["pair"] >= 0
    assert np.array_equal(np.isnan(tau)[keep], ~crossed[keep]), "NaN pattern of tau"
    assert np.array_equal(np.isnan(fsle)[keep], ~crossed[keep]), "NaN pattern of fsle"
    m = keep & crossed
    P, dt = judge["pairs"], abs(float(timestep))
    with np.errstate(invalid="ignore"):
        lvl = P["level"].astype(np.float64)
        slack = 4 * np.finfo(np.float64).eps * lvl * dt
        inside = B["relevant"] & ((lvl - 1) * dt - slack <= tau[:, None]) & (tau[:, None] <= lvl * dt + slack)
        assert np.all(inside.any(axis=1)[m]), "crossing level"
        err_t = np.abs(tau - jt)
        assert np.all(err_t[m] <= B["tau_bound"][m]), f"tau: {np.max((err_t / B['tau_bound'])[m]):.3g} of its bound"
        miss = np.abs(fsle[:, None] - P["fsle"].astype(np.float64)) - B["fsle_bound"]
        miss = np.where(B["relevant"], miss, np.inf).min(axis=1)
        assert np.all(miss[m] <= 0), f"fsle: {int(np.sum(miss[m] > 0))} cells outside every relevant pair's bound"
        jf = judge["fsle"].astype(np.float64)
        single = B["relevant"].sum(axis=1) == 1
        s = m & single
        return dict(cells=int(m.sum()), ambiguous=int((m & ~single).sum()), left_out=float(B["left_out"].mean()),
                    tau_rel=float(np.max((err_t / jt)[m], initial=0.0)), fsle_rel=float(np.max((np.abs(fsle - jf) / jf)[s], initial=0.0)),
                    tau_rel_bound=float(np.max((B["tau_bound"] / jt)[m], initial=0.0)))


# ------------------------------------------------------------------ an analytic record
def global_grid(ny, nx, dtype=np.float64, lat_edge=70.0):
    lat = (np.linspace(-lat_edge, lat_edge, ny) if ny > 1 else np.array([20.0])).astype(dtype)
    lon = (-180.0 + 360.0 / nx * np.arange(nx)).astype(dtype)
    return lat, lon


def smooth_record(seed_lat, seed_lon, n_levels, dtype, gain=1.0):
    """A smooth map that grows with time, wrapped to [-180, 180): level j is the seed grid moved by gain (j / (n_levels - 1))^2
    times (dx, dy) = (25 sin 2y + 9 cos 3x + 6 sin(5x + y), -0.15 y + 5 sin x + 3 cos(4x - 2y)) degrees; level 0 is the seed grid,
    exactly.  Evaluated in longdouble from the seeds as rounded to ``dtype``, then rounded to ``dtype``."""
    lat, lon = np.asarray(seed_lat, dtype=dtype).astype(np.longdouble), np.asarray(seed_lon, dtype=dtype).astype(np.longdouble)
    k = np.longdouble(np.pi) / 180
    X, Y = np.meshgrid(lon, lat)
    dx = 25 * np.sin(2 * Y * k) + 9 * np.cos(3 * X * k) + 6 * np.sin((5 * X + Y) * k)
    dy = -0.15 * Y + 5 * np.sin(X * k) + 3 * np.cos((4 * X - 2 * Y) * k)
    tx, ty = [], []
    for j in range(n_levels):
        a = np.longdouble(gain) * (np.longdouble(j) / (n_levels - 1)) ** 2
        x = X + a * dx
        tx.append((x + 180) % 360 - 180)
        ty.append(Y + a * dy)
    tx, ty = np.stack(tx).astype(dtype), np.stack(ty).astype(dtype)
    tx[tx >= 180] -= 360          # (rounding to float32 can land on +180)
    return np.ascontiguousarray(tx), np.ascontiguousarray(ty)


# the records of tests/test_fsle.py and tests/test_fsle_gpu.py: grid -> gain of smooth_record; 13 levels; three thresholds per call
# in either mode.  The one-seed-wide grids have one kind of pair and need a stronger map to cross at all; on (9, 1) every pair
# starts one spacing apart, so its final separations are the ratios' multiples of it (at 1.05 every one of its nine cells crosses).
GRIDS = {(7, 5): 1.0, (37, 64): 1.0, (33, 130): 1.0, (1, 9): 3.0, (9, 1): 2.5}
N_LEVELS = 13
RATIOS = (1.15, 1.4, 1.8)
DISTANCE_FACTORS = (1.05, 1.3, 1.7)          # times spacing(): metres
DISTANCE_FACTORS_OF = {(9, 1): RATIOS}
TIMESTEP = -3600.0


def case(shape, dtype, mode):
    """``(traj_x, traj_y, seed_lat, seed_lon, thresholds)`` of one test record."""
    lat, lon = global_grid(*shape, dtype)
    tx, ty = smooth_record(lat, lon, N_LEVELS, dtype, GRIDS[shape])
    thr = list(RATIOS) if mode == "ratio" else [f * spacing(lat, lon) for f in DISTANCE_FACTORS_OF.get(shape, DISTANCE_FACTORS)]
    return tx, ty, lat, lon, in_dtype(thr, dtype)


def in_dtype(thresholds, dtype):
    """Thresholds as the library rounds them (to the dtype), as Python floats: what the judge must be given too."""
    return [float(np.dtype(dtype).type(t)) for t in thresholds]


# ------------------------------------------------------------------ hand-worked records (float64)
def meridional_stretch(s, n_levels):
    """phi(t) = phi0 e^{st} on one meridian: a 5 x 1 grid whose N / S pairs grow exactly as e^{st}."""
    lat, lon = np.array([2.0, 4.0, 6.0, 8.0, 10.0]), np.array([30.0])
    ty = (lat[None, :, None] * np.exp(s * np.arange(n_levels))[:, None, None]).copy()
    return np.full_like(ty, 30.0), ty, lat, lon


def tie_case():
    """A 2 x 2 grid at the equator whose cell (0, 0) has an E pair starting 1 degree apart and an N pair starting 2 degrees apart
    that are 2.5 and then 3.5 degrees apart, both, bit for bit: they cross T = 3 degrees of arc at the same time."""
    lat, lon = np.array([0.0, 2.0]), np.array([0.0, 1.0])
    tx, ty = np.empty((3, 2, 2)), np.empty((3, 2, 2))
    tx[:], ty[:] = lon[None, None, :], lat[None, :, None]
    for j, a in ((1, 2.5), (2, 3.5)):
        tx[j, 0, 1], ty[j, 0, 1] = a, 0.0          # the E neighbour, along the equator
        tx[j, 1, 0], ty[j, 1, 0] = 0.0, a          # the N neighbour, along the meridian
    return tx, ty, lat, lon, R_EARTH * (np.pi / 180) * 3.0


def seam_case():
    """One row on the equator, columns at -180, -90, 0, 90; the last parcel drifts west by 5 degrees a level: its separation
    from the first, across the seam, is 90, 95, 100, 105 degrees while the raw longitude difference shrinks."""
    lat, lon = np.array([0.0]), np.array([-180.0, -90.0, 0.0, 90.0])
    tx = np.broadcast_to(lon[None, None, :], (4, 1, 4)).copy()
    tx[:, 0, 3] = 90.0 - 5.0 * np.arange(4)
    return tx, np.zeros_like(tx), lat, lon


def hand_cases():
    """``(traj_x, traj_y, seed_lat, seed_lon, thresholds, mode, cyclic)`` of the hand-worked records, for the kernels too."""
    tx, ty, lat, lon = meridional_stretch(0.11, N_LEVELS)
    yield tx, ty, lat, lon, [1.3, 2.0, 3.5, 4.0], "ratio", False
    nan = ty.copy()
    nan[7, 2, 0] = np.nan
    yield tx, nan, lat, lon, [2.0], "ratio", False
    tx, ty, lat, lon, thr = tie_case()
    yield tx, ty, lat, lon, [thr], "distance", False
    tx, ty, lat, lon = seam_case()
    yield tx, ty, lat, lon, [1.1], "ratio", True
    yield tx, ty, lat, lon, [1.1], "ratio", False


def spacing(seed_lat, seed_lon, radius=R_EARTH):
    """The median initial separation over the pairs of a grid, in metres (what the distance-mode thresholds are multiples of)."""
    d0 = seed_separations(seed_lat, seed_lon, np.float64, True, radius)
    return float(np.nanmedian(d0[d0 > 0]))


# ------------------------------------------------------------------ end to end: small analytic winds and the oracle's record
POS_ATOL64 = 1e-9       # degrees: float64 positions of the advect routes against the oracle (tests/test_gpu_parity.py)
E2E = dict(timestep=-21600.0, SETTLS_order=2)


def vortex_record(nt=9):
    """A global 24 x 48 wind (4 x 7.5 degrees) from ``flows.ideal_vortex``, float64: ``(u, v, lat, lon)``."""
    from lagrangiancoherence_amd import flows
    return flows.ideal_vortex(lat_min=-46, lat_max=50, lon_min=-180, lon_max=180, dx=7.5, dy=4, nt=nt, max_intensity=40, radius=8,
                              center=[-170, 10], u_c=1.0, v_c=0.5, basic_zonal=8, k=0)


def regional_record(nt=9):
    """A weak vortex on a regional 24 x 48 box (0.5 degree), float64: parcels move a few degrees in the record."""
    from lagrangiancoherence_amd import flows
    return flows.ideal_vortex(lat_min=4, lat_max=16, lon_min=-60, lon_max=-36, dx=0.5, dy=0.5, nt=nt, max_intensity=1.5, radius=3,
                              center=[-48, 10], u_c=0.2, v_c=0.1, basic_zonal=0.2, k=0)


def position_error_margin(D, pos_atol=POS_ATOL64, radius=R_EARTH) -> float:
    """What a position error of ``pos_atol`` degrees in each coordinate of both parcels can move a pair's separation by,
    relative to the smallest separation of the record ``D``: each parcel moves by at most sqrt(2) pos_atol of arc."""
    d = np.asarray(D, dtype=np.float64)
    return float(2 * np.sqrt(2) * pos_atol * (np.pi / 180) * radius / np.min(d[np.isfinite(d) & (d > 0)]))
