"""CPU: `state.<observer>.resume = True` for the scores, the duration curves, the event outputs and the bands (roger_amd/scores.py,
durations.py, events.py, bands.py, restart.py) through the host package on the oracle double with all four restatements
(tests/observers_resume_reference.py).

Run A is uninterrupted.  Run B writes a restart file every HOUR under daily observer intervals and stops at such a write inside a day and
inside a running rainfall event; run C continues from B's last file to A's end.  With `resume = True`: C's scores and durations files equal
A's in every variable, bit for bit; B's events followed by C's are A's, the event that was running at the restart once, in C, with its true
start; B's band rows followed by C's are A's, the interval that holds the restart among them -- plain and per zone.  With
`resume = False` C gives what it gave before: the running event with event_start = -1, the interrupted interval dropped.  A changed request
and a restart file without the group are errors that say so; several ranks are refused in `initialize`."""
import types

import numpy as np
import pytest

from golden_util import load_case

DAY = 86400
NDAYS = 6
ITEMS = [("prec", "sum"), ("q_ss", "sum"), ("q_sur", "peak"), ("theta_rz", "first"), ("S_rz", "last")]
PROBS = (0.0, 0.25, 0.5, 1.0)
ZONES = np.array([[3, 3, 7, 7], [3, 0, 7, 7], [9, 9, 9, -2], [9, 9, 3, 11]])        # 0 and -2: outside every zone
BAND_MASK = ZONES != 11                                                              # zone 11 stays in the list, empty
SERIES = np.array([[0, 1, 0, 1], [1, -1, 0, 0], [0, 0, 1, 1], [1, 0, -1, 0]])        # two columns are not scored
DUR_MASK = np.array([[1, 1, 0, 1], [1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 1, 1]])


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def same(a, b):
    """Equal shapes, types and bit patterns (a NaN equals the same NaN)."""
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(bits(a), bits(b)))


def observations():
    rng = np.random.default_rng(11)
    obs = {"q_ss": rng.uniform(0.0, 3.0, size=(2, NDAYS)), "theta_rz": rng.uniform(0.2, 0.4, size=(2, NDAYS))}
    obs["q_ss"][0, 1] = obs["theta_rz"][1, 4] = np.nan
    return obs


def script(out, resume, zones=False, **changed):
    """What set_diagnostics asks for: all four observers at daily intervals."""
    cfg = {
        "scores": dict(observations=observations(), aggregation={"theta_rz": "last"}, series=SERIES),
        "durations": dict(variables={"q_ss": np.array([0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0]), "theta_rz": np.linspace(0.05, 0.6, 12)},
                          spells={"theta_rz": ("below", 0.3), "q_ss": ("at_or_above", 0.01)}, mask=DUR_MASK),
        "events": dict(items=ITEMS, n_slots=4),
        "bands": dict(variables=["q_ss", "theta_rz"], aggregation={"theta_rz": "last"}, probabilities=PROBS, mask=BAND_MASK,
                      zones=ZONES if zones else None),
    }
    for key, value in changed.items():
        which, attr = key.split("__")
        cfg[which][attr] = value

    def set_diagnostics(self, state):
        for which, values in cfg.items():
            o = getattr(state, which)
            o.base_output_path, o.resume = str(out), resume
            for k, v in values.items():
                setattr(o, k, v)

    return set_diagnostics


def make_model(out, resume, zones=False, ndays=NDAYS, changed=None, **override):
    import svat_scripts as S
    from roger_amd import roger_routine

    g, names, forcing = load_case("svat_hetero_combo")
    model = S.make_model(S.params_from_golden(g, names), forcing, ndays)
    out.mkdir(exist_ok=True)
    type(model).set_diagnostics = roger_routine(script(out, resume, zones, **(changed or {})))
    model.override_settings = override
    return model


@pytest.fixture(scope="module")
def backend(oracle):
    from observers_resume_reference import resume_double
    from roger_amd import _native

    made = []
    double = resume_double()

    def make(*a, **k):
        made.append(double(*a, **k))
        return made[-1]

    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(_native, "Context", make)
        mp.setattr(_native, "plane_table", lambda: list(zip(oracle.plane_names(), oracle.plane_is_int())))
        yield made


def stop_of(steps):
    """The end of a step on a full hour, inside a day, inside a rainfall event that the next step continues and that is not the run's
    first (B's file holds an event too), on a day that is neither the first nor the last: where B stops."""
    for (e, t1), (e_next, _) in zip(steps, steps[1:]):
        if e > 1 and e_next == e and t1 % 3600 == 0 and t1 % DAY and DAY < t1 < (NDAYS - 1) * DAY:
            return e, t1
    raise AssertionError("the forcing has no rainfall event that spans a full hour inside a day")


def runs_of(backend, root, zones, steps=None):
    """A, B and C with `resume = True`, and C' -- C with `resume = False` from the same file.  steps: [(event id, end of the step)] of
    the run where they are known already (the GPU test's: tests/test_hip_observers_resume.py); else A's double records them."""
    root.mkdir(exist_ok=True)
    a = make_model(root / "a", True, zones)
    a.setup()
    if steps is None:
        ctx, steps = backend[-1], []
        accumulate = ctx._accumulate

        def recording():
            accumulate()
            steps.append((int(ctx.st.scal.event_id[1]), int(ctx.st.scal.time)))

        ctx._accumulate = recording
    a.run()
    event, t_stop = stop_of(steps)
    b = make_model(root / "b", True, zones, runlen=t_stop, write_restart=True, restart_frequency=3600,
                   restart_output_filename=str(root / "b_{itt:0>5d}.restart.h5"))
    b.setup()
    b.run()
    assert int(b.state.variables.time) == t_stop and int(b.state.backend_context.get_scalars().event_id[1]) == event
    fname = root / f"b_{int(b.state.variables.itt):0>5d}.restart.h5"
    assert fname.is_file() and len(list(root.glob("b_*.restart.h5"))) >= 3             # the hourly writes, and the one B stopped at
    out = types.SimpleNamespace(root=root, event=event, t_stop=t_stop, fname=fname, a=a, b=b)
    for tag, resume in (("c", True), ("c_new", False)):
        c = make_model(root / tag, resume, zones, restart_input_filename=str(fname), runlen=NDAYS * DAY - t_stop)
        c.setup()
        assert int(c.state.variables.time) == t_stop
        c.run()
        assert int(c.state.variables.time) == int(a.state.variables.time) and int(c.state.variables.itt) == int(a.state.variables.itt)
        setattr(out, tag, c)
    return out


@pytest.fixture(scope="module")
def plain(backend, tmp_path_factory):
    return runs_of(backend, tmp_path_factory.mktemp("resume") / "plain", False)


@pytest.fixture(scope="module")
def zonal(backend, tmp_path_factory):
    return runs_of(backend, tmp_path_factory.mktemp("resume") / "zonal", True)


def variables(r, tag, kind):
    from roger_amd import nc4lite

    return {k: np.asarray(v[1]) for k, v in nc4lite.read(str(r.root / tag / f"GoldenSVAT.{kind}.nc"))["variables"].items()}


def test_the_restart_file_holds_the_four_groups_beside_the_reference_s(plain):
    from roger_amd import h5lite, restart

    groups = h5lite.read(str(plain.fname))
    assert {"hip_scores", "hip_durations", "hip_events", "hip_bands", "hip_core", "core"} <= set(groups)
    have = [k for k in restart.REFERENCE_RESTART_VARIABLES if k in plain.b.state.var_meta and k not in restart._LATERAL_ONLY]
    assert set(groups["core"]) == set(have) | set(restart.REFERENCE_ONLY_RESTART_VARIABLES)         # what the reference's reader walks
    ev = groups["hip_events"]
    running = [int(s) for s in ev["slots"]]
    assert len(running) == 1 and int(ev["hdr"][running[0], 0]) == plain.event and ev["maps"].shape == (1, len(ITEMS), 16)
    assert int(ev["hdr"][running[0], 2]) >= 0 and int(groups["hip_bands"]["scalars"][1]) == plain.t_stop // DAY
    assert int(groups["hip_scores"]["t_first"]) == 0 and groups["hip_durations"]["spells"].dtype == np.uint32


def test_scores_of_the_continued_run_equal_the_uninterrupted_run_s(plain):
    a, c = variables(plain, "a", "scores"), variables(plain, "c", "scores")
    assert list(a) == list(c) and a["closed"].tolist() == [1] * NDAYS
    for k in a:
        assert same(a[k], c[k]), k
    assert (a["q_ss_n"].T[SERIES < 0] == 0).all() and (a["q_ss_n"].T[SERIES == 0] == NDAYS - 1).all() and (a["q_ss_n"].T[SERIES == 1] == NDAYS).all()
    # without resume: the tail only, as before
    new = variables(plain, "c_new", "scores")
    dropped = -(-plain.t_stop // DAY)
    assert new["closed"].shape == (NDAYS - dropped,) and new["q_ss_n"].max() <= NDAYS - dropped and not same(a["q_ss_sum_sim"], new["q_ss_sum_sim"])


def test_durations_of_the_continued_run_equal_the_uninterrupted_run_s(plain):
    a, c = variables(plain, "a", "durations"), variables(plain, "c", "durations")
    assert list(a) == list(c) and {"q_ss_count", "q_ss_min", "q_ss_max", "q_ss_q", "q_ss_exceed", "theta_rz_longest", "theta_rz_spells", "theta_rz_run"} <= set(a)
    for k in a:
        assert same(a[k], c[k]), k
    on = DUR_MASK.T != 0
    assert (a["q_ss_n"][on] == NDAYS).all() and (a["q_ss_n"][~on] == 0).all() and a["theta_rz_longest"].max() >= 2
    new = variables(plain, "c_new", "durations")
    assert (new["q_ss_n"][on] == NDAYS - -(-plain.t_stop // DAY)).all()                       # without resume: the tail only


def test_events_of_b_followed_by_c_are_the_uninterrupted_run_s(plain):
    a, b, c = (variables(plain, tag, "events") for tag in "abc")
    assert list(a) == list(b) == list(c)
    na, nb = len(a["event_id"]), len(b["event_id"])
    assert nb >= 1 and len(c["event_id"]) >= 1 and plain.event not in b["event_id"] and int(c["event_id"][0]) == plain.event
    for k in a:
        if k in ("x", "y"):
            assert same(a[k], b[k]) and same(a[k], c[k])
            continue
        assert same(a[k], np.concatenate([b[k], c[k]])), k
    # the event that was running at the restart: once, with its true start before the restart and its end behind it
    k = nb
    assert a["event_id"].tolist().count(plain.event) == 1 and na == nb + len(c["event_id"])
    assert 0 <= c["event_start"][0] * DAY < plain.t_stop < c["event_end"][0] * DAY and a["event_steps"][k] == c["event_steps"][0] > 1
    # without resume: event_start = -1 and sums over the steps behind the restart only
    new = variables(plain, "c_new", "events")
    assert int(new["event_id"][0]) == plain.event and new["event_start"][0] == -1.0 and new["event_steps"][0] < c["event_steps"][0]
    assert not same(new["prec_sum"][0], c["prec_sum"][0]) and same(new["S_rz_last"][0], c["S_rz_last"][0])
    for key in new:
        if key not in ("x", "y"):
            assert same(new[key][1:], c[key][1:]), key


@pytest.mark.parametrize("which", ["plain", "zonal"])
def test_band_rows_of_b_followed_by_c_are_the_uninterrupted_run_s(which, request):
    r = request.getfixturevalue(which)
    a, b, c = (variables(r, tag, "bands") for tag in "abc")
    assert list(a) == list(b) == list(c) and ("zone" in a) == (which == "zonal")
    day = r.t_stop // DAY                                                  # the interval that holds the restart
    assert a["interval"].tolist() == list(range(NDAYS)) and b["interval"].tolist() == list(range(day)) and c["interval"].tolist() == list(range(day, NDAYS))
    for k in a:
        if k in ("probability", "zone", "ncells"):
            assert same(a[k], b[k]) and same(a[k], c[k]), k
            continue
        assert same(a[k], np.concatenate([b[k], c[k]])), k
    assert a["Time"].tolist() == [float(d + 1) for d in range(NDAYS)]
    if which == "zonal":
        assert a["zone"].tolist() == [3, 7, 9, 11] and a["ncells"].tolist() == [4, 4, 5, 0] and a["q_ss"].shape == (NDAYS, 4, len(PROBS))
        assert (a["q_ss_n"][:, 3] == 0).all() and (a["q_ss_n"][:, :3] > 0).all()
    else:
        assert (a["q_ss_n"] == int(BAND_MASK.sum())).all()
    # without resume: a new series from the next boundary, the interrupted interval dropped
    new = variables(r, "c_new", "bands")
    assert new["interval"].tolist() == list(range(NDAYS - day - 1)) and new["Time"].tolist() == a["Time"][day + 1:].tolist()
    assert same(new["theta_rz"], a["theta_rz"][day + 1:]) and a["Time"][day] not in np.concatenate([b["Time"], new["Time"]])


def test_without_resume_the_restart_file_holds_no_group_and_resuming_from_it_fails(backend, plain, tmp_path):
    from roger_amd import h5lite

    w = make_model(tmp_path / "w", False, ndays=1, write_restart=True, restart_output_filename=str(tmp_path / "w_{itt:0>5d}.restart.h5"))
    w.setup()
    w.run()
    (fname,) = tmp_path.glob("w_*.restart.h5")
    assert not [g for g in h5lite.read(str(fname)) if g.startswith("hip_") and g not in ("hip_core", "hip_diag")]
    c = make_model(tmp_path / "c", True, restart_input_filename=str(fname))
    with pytest.raises(RuntimeError, match=r"scores: resume = True, but the restart file .*w_\d+\.restart\.h5 holds no group 'hip_scores'.*"
                                           r"set state\.scores\.resume = False"):
        c.setup()


@pytest.mark.parametrize("changed,text", [
    ({"scores__aggregation": {"q_ss": "last", "theta_rz": "last"}},
     r"scores: resume = True, but the restart file .* was written with kinds = \[0, 1\] and this run asks for kinds = \[1, 1\]"),
    ({"events__n_slots": 8}, r"events: .* was written with n_slots = 4 and this run asks for n_slots = 8"),
    ({"events__items": ITEMS[:2]}, r"events: .* was written with items = \['prec sum', 'q_ss sum', 'q_sur peak', .* asks for items = \['prec sum', 'q_ss sum'\]"),
    ({"durations__variables": {"q_ss": np.array([0.0, 0.01, 0.1, 0.5, 1.0, 2.0, 5.0]), "theta_rz": np.linspace(0.05, 0.7, 12)}},
     r"durations: .* was written with edges = an array of shape \(19,\) and this run asks for edges = an array of shape \(19,\), first difference at flat index 8"),
    ({"durations__mask": None}, r"durations: .* was written with mask = an array of shape \(4, 4\) and this run asks for mask = None"),
    ({"bands__probabilities": (0.0, 0.5, 1.0)}, r"bands: .* was written with probabilities = \[0\.0, 0\.25, 0\.5, 1\.0\] and this run asks for probabilities = \[0\.0, 0\.5, 1\.0\]"),
    ({"bands__zones": ZONES}, r"bands: .* was written with zones = None and this run asks for zones = an array of shape \(4, 4\)"),
])
def test_a_changed_request_is_refused_with_the_first_difference(backend, plain, tmp_path, changed, text):
    c = make_model(tmp_path / "c", True, changed=changed, restart_input_filename=str(plain.fname))
    with pytest.raises(RuntimeError, match=text):
        c.setup()


@pytest.mark.parametrize("which,asked", [("scores", dict(observations={"q_ss": np.zeros(3)})), ("durations", dict(variables={"q_ss": [0.0, 1.0]})),
                                         ("events", dict(items=[("q_ss", "sum")])), ("bands", dict(variables=["q_ss"]))])
def test_several_ranks_are_refused_in_initialize(monkeypatch, which, asked):
    import importlib

    from roger_amd import runtime_state
    from roger_amd.state import RogerState

    st = RogerState()
    o = getattr(st, which)
    for k, v in asked.items():
        setattr(o, k, v)
    o.resume = True
    monkeypatch.setattr(type(runtime_state), "proc_num", property(lambda self: 2))
    with pytest.raises(NotImplementedError, match=rf"{which}: resume = True with 2 ranks.*set state\.{which}\.resume = False"):
        importlib.import_module(f"roger_amd.{which}").initialize(st)
