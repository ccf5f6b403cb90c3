"""The LAZY pipelines of the fused step skip the macropore and crack sub-step loops on wavefronts whose columns all infiltrate +0.0
(rh_physics.h: h_inf_mp / h_inf_sc with DryPath<true>; the predicate is a vote over the wavefront's active lanes).  One rh_run_steps
call over a rain event and the dry day behind it must leave every plane and the scalars exactly as the same steps driven routine by
routine (rh_adaptive_dt + rh_step_core + rh_after_timestep, whose kernels keep the loops alone).

1 000 columns: 15 full wavefronts and one of 40 lanes; parameters per block of 96 columns.  The ponded water z0 is emptied at the end of
every step, so which columns are wet inside a step is set by per-column precipitation weights: 0 (the column never sees rain) or 4.

  wavefronts 0-3, 12-14   no column wet               the dry path on every step
  wavefronts 4-7          every column wet            the loops while it rains
  wavefront 8, 9, 10      lane 17 / 0 / 63 alone wet  one lane sends the wavefront through the loops
  wavefront 11            every lane but one wet
  wavefront 15 (40 lanes) its last active lane (column 999) alone wet
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NX, NY = 40, 25
N = NX * NY
SINGLE_WET = (8 * 64 + 17, 9 * 64, 10 * 64 + 63, N - 1)


def prec_weights():
    w = np.zeros(N)
    w[4 * 64: 8 * 64] = 4.0
    w[list(SINGLE_WET)] = 4.0
    w[11 * 64: 12 * 64] = 4.0
    w[11 * 64 + 30] = 0.0
    return w


def params():
    from roger_amd.svat import hetero_params

    p = hetero_params(N, seed=5)
    block = np.arange(N) // 96
    p = {k: np.asarray(v)[block * 96] for k, v in p.items()}
    # the blocks of the single wet lanes: macropores, a matrix the rain outruns, so that those lanes do have water on the surface when
    # the macropore stage begins, and macropores longer than the wetting front gets (a front past a 50 mm macropore leaves it no open
    # length: such a lane infiltrates nothing and would not keep its wavefront off the dry path)
    special = block >= 5
    p["ks"] = np.where(special, np.minimum(p["ks"], 3.0), p["ks"])
    p["dmpv"] = np.where(special, np.maximum(p["dmpv"], 50.0), p["dmpv"])
    p["lmpv"] = np.where(special, np.minimum(np.maximum(p["lmpv"], 500.0), (p["z_soil"] * 0.9).round(0)), p["lmpv"])
    return p


def same_bits(a, b):
    if a.dtype.kind == "f":
        return (a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))
    return a == b


def test_run_steps_over_wet_dry_and_mixed_wavefronts_equals_the_routine_path():
    import hip_util as H
    from roger_amd.forcing import toy_forcing
    from roger_amd.svat import create_svat

    forcing = toy_forcing("heavyrain", ndays=4)   # rain from 02:00 to 14:00 of day 0 (10-minute and hourly steps), day 1 dry (a daily step)
    w, p = prec_weights(), params()
    t_end = 2 * 86400

    # routine by routine, the forcing and parameter hooks on the host
    ref = create_svat(NX, NY, params=p)
    names = [nm for nm, _ in ref.planes[: ref.planes_held]]
    dt_classes, nsteps = set(), 0
    inf_mp_max = np.zeros(N)
    while True:
        s = ref.get_scalars()
        if s.time >= t_end:
            break
        if s.time % 86400 == 0:
            i = s.itt_forc
            s.itt_day = 0
            s.year[1], s.month[1], s.doy[1] = int(forcing["YEAR"][i]), int(forcing["MONTH"][i]), int(forcing["DOY"][i])
            s.itt_forc = i + 144
            ref.set_scalars(s)
            ref.set_forcing_day(forcing["PREC"][i:i + 144][None, :] * w[:, None], np.broadcast_to(forcing["TA"][i:i + 144], (N, 144)),
                                np.broadcast_to(forcing["PET"][i:i + 144], (N, 144)))
        ref.call("rh_adaptive_dt")
        if (s.month[1] != s.month[0]) and (s.itt > 1):
            ref.call("rh_params_surface")
        ref.call("rh_step_core")
        ref.call("rh_after_timestep")
        nsteps += 1
        dt_classes.add(int(ref.get_scalars().dt_secs))
        inf_mp_max = np.maximum(inf_mp_max, ref.download("inf_mp"))
    assert {600, 3600, 86400} <= dt_classes, dt_classes
    assert 30 < nsteps < 200, nsteps
    # the layout is what the docstring says: the single wet lanes had water for their macropores, the dry columns never
    assert (inf_mp_max[list(SINGLE_WET)] > 0).all(), inf_mp_max[list(SINGLE_WET)]
    assert (inf_mp_max[w == 0] == 0).all()
    assert (inf_mp_max[4 * 64: 8 * 64] > 0).any()
    want_scal = H.scalars_to_row(ref.get_scalars())
    want = {nm: ref.download(nm) for nm in names}
    ref.close()

    # the same steps as ONE rh_run_steps call: an eager first step, then the lazy sparse kernel, the last step storing every plane
    ctx = create_svat(NX, NY, params=p)
    ctx.set_forcing_series(forcing)
    ctx.set_forcing_weights(w, np.zeros(N), np.ones(N))
    ctx.run_steps(nsteps)
    s = ctx.get_scalars()
    assert s.sanity_ok == 1
    assert ctx.sparse_steps() > nsteps // 2, ctx.sparse_steps()   # (the lazy sparse kernel ran: the pipeline with the dry paths)
    np.testing.assert_array_equal(H.scalars_to_row(s), want_scal)
    for nm in names:
        got = ctx.download(nm)
        ok = same_bits(got, want[nm])
        assert ok.all(), (nm, np.flatnonzero(~ok)[:10], got[~ok][:5], want[nm][~ok][:5])
    ctx.close()
