"""GPU: the scores, the duration curves, the event outputs and the bands carried through a restart (ABI version 18: rh_scores_restore,
rh_durations_restore, rh_events_state / _restore, rh_bands_state / _restore), bit for bit.

At the C ABI: context A steps N steps with the observer configured.  Context B steps N1 steps and is read out: every plane it holds, the
scalars, the observer's state.  A fresh context C takes B's planes and scalars, is configured like B (the same t_first), restored, and
steps N - N1: its read-out equals A's in every bit.  The columns are the heterogeneous 4 x 4 golden (svat_hetero_combo) as it is and tiled
to 257 x 1 -- one column beyond a 256-column tile and two workgroups' copies of the slots' ids -- under the golden's forcing; N1 lies
inside a day and inside a rainfall event that spans it, asserted from B's scalars.

Through the package: the runs A, B, C of tests/test_observers_resume_host.py on the device, with real restart files, compared by that
file's own checks."""
import ctypes as C
import functools

import numpy as np
import pytest

from golden_util import load_case

pytestmark = pytest.mark.gpu

DAY = 86400
NDAYS = 4
GRIDS = [(4, 4), (257, 1)]
EV_ITEMS = (("prec", 0), ("q_ss", 0), ("q_sur", 1), ("theta_rz", 2), ("S_rz", 3))
PROBS = (0.0, 0.25, 0.5, 1.0)
RH_ERR_ARG, RH_ERR_STATE = -1, -3


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def assert_same(got, want, what):
    assert len(got) == len(want), what
    for k, (g, w) in enumerate(zip(got, want)):
        g, w = np.asarray(g), np.asarray(w)
        assert g.shape == w.shape and g.dtype == w.dtype, (what, k, g.shape, w.shape, g.dtype, w.dtype)
        ok = bits(g) == bits(w)
        assert ok.all(), (what, "part", k, np.argwhere(~ok)[:5], g[~ok][:3], w[~ok][:3])


def make_ctx(nx, ny):
    """The golden's 16 columns tiled over nx x ny, at the golden's initial state and clock; (context, forcing driver, forcing)."""
    import hip_util as H
    from roger_amd import _native as N

    g, names, forcing = load_case("svat_hetero_combo")
    ctx = N.Context(nx, ny, enable_lateral_flow=0)
    for row, nm in zip(g["state0"], names):
        if H._held(ctx, nm):
            ctx.upload(nm, np.resize(row, nx * ny))
    ctx.set_scalars(H.scalars_from_row(g["scal0"]))
    ctx.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    return ctx, H.HipForcingDriver(ctx, forcing), forcing


def advance(ctx, drv, nsteps):
    for _ in range(nsteps):
        ctx.step(drv.before_step())


@functools.lru_cache(maxsize=None)
def clock(nx, ny):
    """[(event id, end of the step)] of a context without observers over NDAYS days, and N1: the number of steps after which the clock
    is inside a day and inside an event (not the run's first) that the next step continues."""
    ctx, drv, _ = make_ctx(nx, ny)
    steps = []
    while not steps or steps[-1][1] < NDAYS * DAY:
        advance(ctx, drv, 1)
        s = ctx.get_scalars()
        assert s.sanity_ok == 1
        steps.append((int(s.event_id[1]), int(s.time)))
    ctx.close()
    for k, ((e, t1), (e_next, _)) in enumerate(zip(steps, steps[1:])):
        if e > 1 and e_next == e and t1 % DAY and t1 > DAY:
            return steps, k + 1
    raise AssertionError("the forcing has no rainfall event that spans the end of a step inside a day")


def tiled(a, n):
    return np.resize(np.asarray(a).reshape(-1), n)


class Scores:
    series = np.array([0, 1, 0, 1, 1, -1, 0, 0, 0, 0, 1, 1, 1, 0, -1, 0])        # two of sixteen columns are not scored

    def __init__(self, n):
        rng = np.random.default_rng(11)
        self.obs = np.stack([rng.uniform(0.0, 9.0, size=(2, NDAYS)), rng.uniform(0.0, 3.0, size=(2, NDAYS)), rng.uniform(0.2, 0.4, size=(2, NDAYS))])
        self.obs[0, 0, 1] = self.obs[2, 1, 2] = np.nan
        self.map = tiled(self.series, n).astype(np.int32)

    def configure(self, ctx, resumed=False):
        now = int(ctx.get_scalars().time)
        ctx.scores_configure(("prec", "q_ss", "theta_rz"), (0, 0, 1), self.obs, self.map, DAY, -(-now // DAY) * DAY if resumed else 0)

    def read(self, ctx):
        return ctx.scores_read()

    def restore(self, ctx, held):
        ctx.scores_restore(held[0], held[1], 0)

    def check_b(self, held):
        assert held[1].tolist()[:1] == [1] and not held[1][-1] and np.any(held[0][:2, 0] != 0)    # a day closed, and a sum under way


class Durations:
    mask = np.array([1, 1, 0, 1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1])

    def __init__(self, n):
        self.on = tiled(self.mask, n).astype(np.uint8)
        self.edges = [np.array([0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0]), np.linspace(0.05, 0.6, 12)]
        self.spells = [(1, 0.01), (0, 1.0)]          # q_ss at or above 0.01 mm a day; theta_rz below 1: its run is always under way

    def configure(self, ctx, resumed=False):
        ctx.durations_configure(("q_ss", "theta_rz"), (0, 1), self.edges, self.spells, self.on, DAY, 0)

    def read(self, ctx):
        counts, vals, spells = ctx.durations_read()
        return (*counts, vals, spells)

    def restore(self, ctx, held):
        ctx.durations_restore(held[:2], held[2], held[3])

    def check_b(self, held):
        run, numbers = held[3][1, 0], (self.on != 0) & (held[1][-1] == 0) & (held[2][1, 2] < 1.0)   # (a NaN theta_rz is in no spell)
        assert 2 * numbers.sum() > run.size and (run[numbers] > 0).all() and (run[self.on == 0] == 0).all(), "the spell of theta_rz is not under way at N1"


class Events:
    slots = 4

    def __init__(self, n):
        pass

    def configure(self, ctx, resumed=False):
        ctx.events_configure([v for v, _ in EV_ITEMS], [k for _, k in EV_ITEMS], self.slots)

    def read(self, ctx):
        hdr, values, lost = ctx.events_read(slots=range(self.slots))
        ids, running, drained = ctx.events_state()
        return hdr, np.stack([values[s] for s in range(self.slots)]), np.array([int(lost), running, drained]), ids

    def restore(self, ctx, held):
        hdr, maps, (lost, running, drained), ids = held
        live = {s: maps[s] for s in range(self.slots) if hdr[s, 0] > drained}
        assert live
        ctx.events_restore(hdr, ids, running, drained, bool(lost), live)

    def check_b(self, held):
        hdr, maps, (lost, running, drained), ids = held
        assert running == 0 and not lost and (ids == hdr[:, 0]).all() and (hdr[:, 0] > 0).sum() >= 2


class Bands:
    mask = np.array([1, 1, 1, 0, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 1, 1])
    zones = np.array([0, 1, 0, 1, -1, 1, 0, 0, 1, 1, 0, -1, 0, 1, 0, 1])         # zones 0 and 1 of three: zone 2 is empty

    def __init__(self, n, zonal=False):
        self.zonal, self.n = zonal, n

    def configure(self, ctx, resumed=False):
        kw = dict(zones=tiled(self.zones, self.n), n_zones=3) if self.zonal else dict(mask=tiled(self.mask, self.n))
        ctx.bands_configure(("prec", "q_ss", "theta_rz"), (0, 0, 1), PROBS, DAY, 0, capacity=8, **kw)

    def rows(self, ctx, first):
        n = ctx.bands_count() - first
        return ctx.bands_zonal_read(first, n) if self.zonal else ctx.bands_read(first, n)

    def read(self, ctx, first=0):
        return (*self.rows(ctx, first), ctx.bands_state(), np.array([ctx.bands_count()]))

    def restore(self, ctx, held):
        ctx.bands_restore(held[-2], int(held[-1][0]))

    def check_b(self, held):
        assert held[-1][0] >= 1 and np.any(held[-2][:2] != 0)                                    # rows, and a sum under way


class ZonalBands(Bands):
    def __init__(self, n):
        super().__init__(n, zonal=True)


def continued(nx, ny, obs, n1, nsteps):
    """B over n1 steps, read out; C from B's planes, scalars and observer state over the rest: (B's read-out, C's, C's context)."""
    import hip_util as H

    b, drv, forcing = make_ctx(nx, ny)
    obs.configure(b)
    advance(b, drv, n1)
    s = b.get_scalars()
    assert int(s.time) % DAY != 0 and int(s.event_id[1]) > 0, "N1 is not inside a day and inside an event"
    held = obs.read(b)
    planes = {nm: b.download(nm) for nm, _ in b.planes[: b.planes_held]}
    b.close()
    g, _, _ = load_case("svat_hetero_combo")
    from roger_amd import _native as N

    c = N.Context(nx, ny, enable_lateral_flow=0)
    for nm, a in planes.items():
        c.upload(nm, a)
    c.set_scalars(s)
    c.set_luts(g["lut_ilu"], g["lut_gc"], g["lut_gcm"], g["lut_rdlu"])
    i0 = int(s.itt_forc) - 144                                      # mid-day: the day's forcing B took at midnight
    c.set_forcing_day(*[forcing[v][i0:i0 + 144] for v in ("PREC", "TA", "PET")])
    obs.configure(c, resumed=True)
    obs.restore(c, held)
    advance(c, H.HipForcingDriver(c, forcing), nsteps - n1)
    return held, c


@pytest.mark.parametrize("kind", [Scores, Durations, Events, Bands, ZonalBands])
@pytest.mark.parametrize("nx,ny", GRIDS)
def test_a_restored_context_ends_with_the_uninterrupted_context_s_state(nx, ny, kind):
    steps, n1 = clock(nx, ny)
    obs = kind(nx * ny)
    a, drv, _ = make_ctx(nx, ny)
    obs.configure(a)
    advance(a, drv, len(steps))
    want = obs.read(a)
    held, c = continued(nx, ny, obs, n1, len(steps))
    obs.check_b(held)
    what = f"{kind.__name__} {nx} x {ny}, restart after step {n1} of {len(steps)}"
    assert int(c.get_scalars().time) == int(a.get_scalars().time) == steps[-1][1]
    for nm, _ in a.planes[: a.planes_held]:                             # (the step itself continues bit for bit: tests/test_hip_restart.py)
        assert_same([c.download(nm)], [a.download(nm)], f"{what}: plane {nm}")
    if isinstance(obs, Bands):
        rows_b = int(held[-1][0])
        got = obs.read(c, first=rows_b)
        nparts = len(want) - 2
        assert int(want[-1][0]) == NDAYS and want[0][:, 0].tolist() == list(range(NDAYS)) and 1 <= rows_b < NDAYS
        assert_same([np.concatenate([held[k], got[k]]) for k in range(nparts)] + list(got[-2:]), want, what)
        if obs.zonal:
            assert (want[1][:, :, 2] == 0).all() and (want[1][:, :, :2, 0] > 0).all() and np.isnan(want[2][:, :, 2]).all()
    else:
        assert_same(obs.read(c), want, what)
    if kind is Scores:
        assert want[1].tolist() == [1] * NDAYS and not want[0][:, :, obs.map < 0].any() and np.any(want[0][:, 1:] != 0)
    if kind is Events:
        hdr = want[0]
        e = steps[n1 - 1][0]
        slot = e % obs.slots
        assert hdr[slot, 0] == e and 0 <= hdr[slot, 2] < steps[n1 - 1][1] < hdr[slot, 3]       # the true start, before the restart
    a.close()
    c.close()


def test_the_restore_calls_refuse_by_return_code():
    """Before the configuration RH_ERR_STATE; wrong sizes RH_ERR_ARG and nothing is copied; after a step has run RH_ERR_STATE."""
    nx, ny = 4, 4
    n = nx * ny
    ctx, drv, _ = make_ctx(nx, ny)
    lib, h = ctx._lib, ctx._h
    vp = lambda a: a.ctypes.data_as(C.c_void_p)   # noqa: E731
    kinds = {k.__name__: k(n) for k in (Scores, Durations, Events, Bands)}
    m, cl = np.ones((3, 5, n)), np.ones(NDAYS, dtype=np.uint8)
    cnt, vals, sp = np.ones((9 + 14, n), dtype=np.uint32), np.ones((2, 3, n)), np.ones((2, 3, n), dtype=np.uint32)
    hdr, ids = np.full((4, 6), 7, dtype=np.int64), np.full(4, 7, dtype=np.int64)
    slots, maps = np.array([1], dtype=np.int32), np.ones((1, len(EV_ITEMS), n))
    acc = np.ones((3, n))
    calls = {
        "Scores": lambda m=m, cl=cl, t=0: lib.rh_scores_restore(h, vp(m), m.nbytes, vp(cl), cl.nbytes, t),
        "Durations": lambda cnt=cnt, vals=vals: lib.rh_durations_restore(h, vp(cnt), cnt.nbytes, vp(vals), vals.nbytes, vp(sp), sp.nbytes),
        "Events": lambda hdr=hdr, maps=maps, slots=slots: lib.rh_events_restore(h, vp(hdr), hdr.nbytes, vp(ids), ids.nbytes, 0, 0, 0, vp(slots), len(slots),
                                                                              vp(maps), maps.nbytes),
        "Bands": lambda acc=acc, rows=3: lib.rh_bands_restore(h, vp(acc), acc.nbytes, rows),
    }
    for name, call in calls.items():
        assert call() == RH_ERR_STATE, (name, "before the configuration")
    for obs in kinds.values():
        obs.configure(ctx)
    before = {name: obs.read(ctx) for name, obs in kinds.items()}
    wrong = {
        "Scores": [dict(m=m[:1]), dict(cl=cl[:-1]), dict(t=3600), dict(t=-DAY)],
        "Durations": [dict(cnt=cnt[:-1]), dict(vals=vals[:1])],
        "Events": [dict(hdr=hdr[:3]), dict(maps=maps[:, :-1]), dict(slots=np.array([4], dtype=np.int32))],
        "Bands": [dict(acc=acc[:1]), dict(rows=-1)],
    }
    for name, cases in wrong.items():
        for kw in cases:
            assert calls[name](**kw) == RH_ERR_ARG, (name, list(kw))
        assert_same(kinds[name].read(ctx), before[name], f"{name}: a refused restore copied something")
    for name, call in calls.items():                                        # as they are, they are accepted ...
        assert call() == 0, (name, ctx._lib.rh_last_error(h))
    assert ctx.scores_read()[0].min() == 1.0 and ctx.events_state()[0].tolist() == [7] * 4 and ctx.bands_count() == 3
    advance(ctx, drv, 1)
    for name, call in calls.items():                                        # ... until a step has run
        assert call() == RH_ERR_STATE, (name, "after a step")
        assert b"a step has run since" in ctx._lib.rh_last_error(h)
    ctx.close()


@pytest.fixture(scope="module")
def package_runs(tmp_path_factory):
    """A, B, C and C' of tests/test_observers_resume_host.py on the device, all four observers at once, 4 x 4."""
    import test_observers_resume_host as T
    from roger_amd import runtime_settings as rs

    object.__setattr__(rs, "diskless_mode", False)   # (runtime settings are locked once the core modules are imported)
    root = tmp_path_factory.mktemp("resume_device")
    probe = T.make_model(root / "probe", False)          # the run's clock, step by step: where B can stop
    probe.setup()
    steps = []
    while not steps or steps[-1][1] < T.NDAYS * DAY:
        probe.step(probe.state)
        s = probe.state.backend_context.get_scalars()
        steps.append((int(s.event_id[1]), int(s.time)))
    return {zones: T.runs_of(None, root / ("zonal" if zones else "plain"), zones, steps=steps) for zones in (False, True)}


@pytest.mark.parametrize("which", ["scores", "durations", "events", "bands", "bands_zonal", "file"])
def test_a_script_continued_from_a_real_restart_file(package_runs, which, request):
    import test_observers_resume_host as T

    plain, zonal = package_runs[False], package_runs[True]
    if which == "scores":
        T.test_scores_of_the_continued_run_equal_the_uninterrupted_run_s(plain)
    elif which == "durations":
        T.test_durations_of_the_continued_run_equal_the_uninterrupted_run_s(plain)
    elif which == "events":
        T.test_events_of_b_followed_by_c_are_the_uninterrupted_run_s(plain)
    elif which == "file":
        T.test_the_restart_file_holds_the_four_groups_beside_the_reference_s(plain)
    else:
        name = "zonal" if which == "bands_zonal" else "plain"
        T.test_band_rows_of_b_followed_by_c_are_the_uninterrupted_run_s(name, types_request({"plain": plain, "zonal": zonal}))


def types_request(values):
    """What the CPU file's bands test asks of pytest's `request`: the runs by name."""
    import types

    return types.SimpleNamespace(getfixturevalue=values.__getitem__)
