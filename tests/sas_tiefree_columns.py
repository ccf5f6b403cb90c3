"""Tie-free columns for the offline transport step: problems on which every column owes the oracle 1e-10 in every output, with no
allowance.  tests/test_sas_tiefree_reference.py shows on the CPU that the reference alone meets the conditions below,
tests/test_hip_sas_tiefree.py holds the device to them, tools/sas_branches.py lists the branch directions they take.

A residue tie (sas_binding.FIRST_TIE) needs a decision that the last bit of Omega can flip: a flux that takes all
the water of an age class (the class keeps 0 or 1e-16 mm), a snap to zero, a class that ends a day next to 1e-8 mm.  The oracle reports
how far a column's day stayed from every such decision (oc_sas_step_margin, SasState.step_oracle(margin=True)); a column is TIE-FREE on
a day when that margin is at least TIEFREE_MARGIN = 1e-6, six decades above the kernel's rounding differences.  The margin is a
condition on the inputs, not a tolerance on the kernel.

tiefree_problem draws columns that keep the margin by construction:

state      about 15 % of the age classes are exactly empty, class 0 among them, and the SAME classes in root zone and subsoil: water that
           percolates or rises joins a class that holds water already, so no class starts with a trace.  Every other class holds
           0.8 .. 2 mm (the subsoil 1.5 times that), the oldest a fifth of the store: the kumaraswami function with b < 1 is infinitely
           steep at the top, and an oldest class of ordinary size would turn an ulp of the cumulative StorAge into 1e-8 of Omega.
           Classes 1, mid - 2 .. mid and the oldest are never empty (the dirac thresholds, below).
fluxes     every outgoing flux is 0 (one column in five) or 0.02 .. 0.08 mm a day: the youngest class under the steepest function
           (Omega ~ 2.5 x^0.2) loses a tenth of its water to one flux.  60 % of the columns are wet: 2 .. 15 mm of matrix infiltration
           or 1 .. 5 mm through the large pores or both, and 1 .. 3 mm into the subsoil or none; a dry column has none of the three.
           A wet column without infiltration into the subsoil has no percolation out of the root zone (it would found the subsoil's
           class 0 with a trace); either flux has its zero case elsewhere.
SAS codes  VARIANTS, one per (column, flux), rotated by column, flux and configuration: 1, 2, 3, 31 .. 37, 4, 51, 52, 6 with a free
           exponent and with exactly 0.5, 1.5, 1.0 and 0.2, 61, 62.  Under Euler and RK4 all but the gamma function (EXPLICIT_VARIANTS
           says why).
bounds     p5 and p6 per column and flux from the store the flux leaves, in turn: S < p5 (S_rel < 0), p5 < S < p6, S > p6 (S_rel > 1).
dirac      thresholds from {-1, 0, 1, mid, ages - 1, ages, ages + 5}.  -1 and the two at or above `ages` select nothing.  The others
           take the whole (small) flux from one class, which holds at least ten times that or is exactly empty (class 0 and, a day
           later, class 1 of a dry column: nothing is taken, on both sides): a piston that does not empty its class is tie-free.
           The threshold of a (column, flux) rotates with column, flux and configuration.
special    columns 2 and n - 2 have maskCatch = 0 (one column is one workgroup: a workgroup of every shape sees only a masked column);
           column 5 holds and receives a signal above d18O_max (every delta is NaN), column 6 receives one below d18O_min into an
           ordinary store, columns 9 and 10 hold and receive one 0.05 permil inside the upper and 0.001 permil inside the lower bound.
           (The bounds of the delta notation are part of the margin.  The upper bound is 0 permil, where the notation cancels: an ulp
           of a concentration is 1000 * 2^-52 = 2.2e-13 permil, a mean of equal values summed in another order moves by a few ulps, and
           atol 1e-12 alone would hold the device to the last bit there; at -0.05 the tolerance is 6e-12, some thirty ulps.)
           Column 12 is unlabelled: a signal of exactly 0 in every class of both stores and in the inflow, so every flux's mean
           signal is exactly 0 and `conc != 0 ? conc : NaN` takes its NaN arm.  Under Euler and RK4 column 13 is wet through all
           three infiltration fluxes with C_in = NaN: the NaN guards of the explicit inflow take their NaN arm, for isotopes and
           anions.  Under Euler on isotopes column 11 has the five oldest classes of both stores empty and the oldest with the
           NaN marker that ageing leaves in an empty oldest class (msa[-1] = nan where sa <= 0); its percolation and capillary rise
           are pistons with threshold ages - 1, its other fluxes uniform.  A piston over an empty class has tt = 1 there and takes
           nothing (the update clips to the class's 0 mm), and mtt = where(tt > 0, msa, 0) reads that class's signal.  It is NOT
           NaN: the inflow that opens every sub-step mixes each class's signal with weight sa / (dsa + sa), and `tot > 0` false
           gives 0, so the marker of an empty class is gone before any flux reads it.  That is why the `isnan(mtt)` guards of the
           explicit update cannot take their NaN arm from a state the solvers leave; the column holds the wipe itself, which the
           kernels restate as `(msa != msa) ? 0 : msa`.  Under the anion kernels columns 1, 7, 13, .. are crops above and below 80 % of the root zone's saturation
           storage in turn, and every third column has partition coefficients of exactly 1.

SEEDS: a configuration's seed is 1000 * nages + substeps (seed_of); no configuration needed another one."""
import numpy as np

from sas_binding import FLUXES, ISOTOPE_CONSTANTS, SasState

TIEFREE_MARGIN = 1e-6
SPECIAL = {"above": 5, "below_in": 6, "inside_hi": 9, "inside_lo": 10, "unlabelled": 12, "nan_in": 13, "nan_mtt": 11}   # special columns (above)
NAN_MTT_EMPTY = 5         # empty classes at the top of both stores of the NaN-marker column: empty through three days of ageing
INSIDE_HI = 0.05          # permil below d18O_max (special columns, above)
# (code, exponent or None for a free draw)
VARIANTS = ((1, None), (2, None), (3, None), (31, None), (32, None), (33, None), (34, None), (35, None), (36, None), (37, None),
            (4, None), (51, None), (52, None), (6, None), (6, 0.5), (6, 1.5), (6, 1.0), (6, 0.2), (61, None), (62, None))
# The explicit solvers normalise a flux's clipped increments of Omega by their sum (calc_TT_num_nonneg).  The gamma function's Omega drops
# from its last value to 0 at the top edge, that negative increment passes the limiter (the oldest class holds more), and the sum
# cancels to rounding noise: the reference's own distribution is 1e10 or inf there.  No column with code 4 is tie-free under Euler or
# RK4 (the margin says so: the update that follows clips every class), so their problems draw the other nineteen variants.
EXPLICIT_VARIANTS = tuple(v for v in VARIANTS if v[0] != 4)
CODES = tuple(sorted({c for c, _ in VARIANTS}))
SOURCE = {"evap_soil": "rz", "transp": "rz", "q_rz": "rz", "q_ss": "ss", "cpr_rz": "ss"}   # the store a flux leaves

# nages = ages + 1 is what both launchers compare (rh_sas_kernels.h, rh_sas_solvers_impl.h): the last age axis of every shape, the
# first of the next, the one before (whose last thread holds one class less), an interior point of the largest shape and its last axis
DET_NAGES = (63, 64, 65, 127, 128, 129, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3001, 4096)
EXPLICIT_NAGES = (63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 2047, 2048, 2049, 3001, 4096)
DET_LAST = (64, 128, 256, 512, 1024, 2048, 4096)          # the last axis of each shape of the deterministic launcher
EXPLICIT_LAST = (64, 256, 512, 1024, 2048, 4096)          # ... of the explicit solvers'
STAGED_NAGES = (64, 65, 512, 513, 1024, 1025)
SUBSTEPS = (2, 3, 6)
NDAYS = 3


def _cfg(nages_list, tracer, solver):
    """(n, ages, substeps, stats, tracer, solver) per age axis: sub-steps in turn, age statistics for every other one."""
    return [(16 if na > 2049 else 32, na - 1, SUBSTEPS[j % 3], j % 2 == 0, tracer, solver) for j, na in enumerate(nages_list)]


# configuration groups: the SAS codes of a group cover every flux (test_sas_tiefree_reference.py)
GROUPS = {
    "deterministic": _cfg(DET_NAGES, "oxygen18", "deterministic"),
    "Euler": _cfg(EXPLICIT_NAGES, "oxygen18", "Euler"),
    "RK4": _cfg(EXPLICIT_NAGES, "oxygen18", "RK4"),
    "bromide": _cfg(DET_LAST, "bromide", "deterministic"),
    "chloride": _cfg(DET_LAST, "chloride", "deterministic"),
    "virtualtracer": _cfg(DET_LAST, "virtualtracer", "deterministic"),
    "bromide-Euler": _cfg(EXPLICIT_LAST, "bromide", "Euler"),
    "bromide-RK4": _cfg(EXPLICIT_LAST, "bromide", "RK4"),
}
STAGED = _cfg(STAGED_NAGES, "oxygen18", "deterministic")
CONFIGS = [c for g in GROUPS.values() for c in g]


def cfg_id(c):
    n, ages, substeps, stats, tracer, solver = c
    return f"{tracer}-{solver}-a{ages}-s{substeps}-{'stats' if stats else 'nostats'}"


def seed_of(c):
    return 1000 * (c[1] + 1) + c[2]


def conc_of_delta(delta, tracer="oxygen18"):
    """The concentration whose delta value is `delta` (the inverse of conc_to_delta, transport.py:315-340)."""
    v = ISOTOPE_CONSTANTS["deuterium" if tracer == "deuterium" else "oxygen18"][0]
    r = v * (delta / 1000.0 + 1.0)
    return r / (1.0 + r)


def variants_for(solver):
    return VARIANTS if solver == "deterministic" else EXPLICIT_VARIANTS


def codes_for(solver):
    return tuple(sorted({c for c, _ in variants_for(solver)}))


def variant_of(n, seed, count):
    """Index into a list of `count` variants per (column, flux)."""
    i = np.arange(n)[:, None]
    f = np.arange(len(FLUXES))[None, :]
    return (i + 3 * f + 7 * (seed // 1000) + seed % 1000) % count


def dirac_thresholds(ages):
    return (-1.0, 0.0, 1.0, float(ages // 2), float(ages - 1), float(ages), float(ages + 5))


def tiefree_problem(n, ages, substeps, seed, tracer="oxygen18", solver="deterministic", stats=False):
    rng = np.random.default_rng(seed)
    st = SasState(n, ages, substeps, stats, tracer=tracer, solver=solver)
    mid = ages // 2
    empty = rng.uniform(size=(n, ages)) < 0.15
    empty[:, 0] = True
    empty[:, [1, mid - 2, mid - 1, mid, ages - 1]] = False
    special = SPECIAL
    lo, hi = ISOTOPE_CONSTANTS["oxygen18"][1:]
    for key, scale in (("rz", 1.0), ("ss", 1.5)):
        sa = np.where(empty, 0.0, rng.uniform(0.8, 2.0, (n, ages)) * scale)
        sa[:, -1] = 0.25 * sa[:, :-1].sum(axis=1)            # a fifth of the store
        st.state[f"sa_{key}"][:] = sa
        if st.anion:
            msa = np.where(sa > 0, sa * rng.uniform(0.005, 0.02, (n, ages)), 0.0)     # solute mass by age
        else:
            msa = np.where(sa > 0, rng.uniform(0.00197, 0.00200, (n, ages)), 0.0)
            msa[special["above"]] = np.where(sa[special["above"]] > 0, conc_of_delta(hi + 24.0), 0.0)
            msa[special["inside_hi"]] = np.where(sa[special["inside_hi"]] > 0, conc_of_delta(hi - INSIDE_HI), 0.0)
            msa[special["inside_lo"]] = np.where(sa[special["inside_lo"]] > 0, conc_of_delta(lo + 1e-3), 0.0)
            msa[special["unlabelled"]] = 0.0
        st.state[f"msa_{key}"][:] = msa
        if has_nan_mtt(tracer, solver):      # the top classes empty, the oldest with the NaN marker that ageing leaves in an empty one
            st.state[f"sa_{key}"][special["nan_mtt"], -NAN_MTT_EMPTY:] = 0.0
            st.state[f"msa_{key}"][special["nan_mtt"], -NAN_MTT_EMPTY:] = 0.0
            st.state[f"msa_{key}"][special["nan_mtt"], -1] = np.nan
    S = {k: st.state[f"sa_{k}"].sum(axis=1) for k in ("rz", "ss")}

    wet = rng.uniform(size=n) < 0.6
    inf_mat = np.where(wet, rng.uniform(2, 15, n), 0) * (rng.uniform(size=n) < 0.85)
    inf_pf = np.where(wet, rng.uniform(1, 5, n), 0) * (rng.uniform(size=n) < 0.5)
    inf_mat = np.where(wet & (inf_mat == 0) & (inf_pf == 0), 3.0, inf_mat)
    inf_ss = np.where(wet, rng.uniform(1, 3, n), 0) * (rng.uniform(size=n) < 0.5)
    if solver != "deterministic":         # the column whose inflow carries NaN: all three infiltration fluxes, so each guard meets it
        wet[special["nan_in"]] = True
        inf_mat[special["nan_in"]], inf_pf[special["nan_in"]], inf_ss[special["nan_in"]] = 6.0, 2.0, 1.5
    st.inp["inf_mat_rz"][:], st.inp["inf_pf_rz"][:], st.inp["inf_pf_ss"][:] = inf_mat, inf_pf, inf_ss
    for f in FLUXES:
        st.inp[f][:] = rng.uniform(0.02, 0.08, n) * (rng.uniform(size=n) < 0.8)
    st.inp["q_rz"][wet & (inf_ss == 0)] = 0.0
    C_in = rng.uniform(0.00197, 0.00200, n)
    if st.anion:
        C_in = rng.uniform(0.0, 0.05, n)
    else:
        C_in[special["above"]] = conc_of_delta(hi + 24.0)
        C_in[special["below_in"]] = conc_of_delta(lo - 30.0)
        C_in[special["inside_hi"]] = conc_of_delta(hi - INSIDE_HI)
        C_in[special["inside_lo"]] = conc_of_delta(lo + 1e-3)
        C_in[special["unlabelled"]] = 0.0
    if solver != "deterministic":
        C_in[special["nan_in"]] = np.nan
    st.inp["C_in"][:] = C_in
    st.maskCatch[:] = 1
    st.maskCatch[[2, n - 2]] = 0

    variants = variants_for(solver)
    var = variant_of(n, seed, len(variants))
    thresholds = dirac_thresholds(ages)
    for j, f in enumerate(FLUXES):
        p = st.sas[f]
        code = np.array([variants[v][0] for v in var[:, j]], dtype=float)
        fixed = np.array([variants[v][1] if variants[v][1] is not None else np.nan for v in var[:, j]])
        p[:, 0] = code
        p[:, 1] = np.where(np.isnan(fixed), rng.uniform(0.2, 2.5, n), fixed)                      # power-law exponent; kumaraswami a
        p[:, 2] = rng.uniform(0.5, 2.5, n)                                                        # kumaraswami b
        p[:, 3] = rng.uniform(0.2, 0.8, n)
        p[:, 4] = rng.uniform(0.5, 1.5, n)
        is2, is4, is5 = code == 2, code == 4, (code == 51) | (code == 52)
        thr = np.array(thresholds)[(np.arange(n) + j + seed % 1000 + seed // 1000) % len(thresholds)]
        if solver == "RK4":
            # RK4's third trial update clips with the sign as written (`sarkn - dsarkn < 0`): a piston on an exactly empty class leaves
            # a NEGATIVE trial StorAge there, and the fourth evaluation founds a trace class from it.  A dry column's classes 0 and 1
            # are empty, so under RK4 its pistons take the mid threshold instead.  (Euler keeps them: nothing is taken.)
            thr = np.where(~wet & ((thr == 0) | (thr == 1)), float(mid), thr)
        p[is2, 1] = thr[is2]
        p[is4, 1] = rng.choice([0.5, 1.0, 1.7, 3.0], n)[is4]                                      # gamma: shape, scale
        p[is4, 2] = rng.choice([0.3, 1.0, 2.0, 5.0, 12.0], n)[is4]
        p[is5, 1] = rng.uniform(0.5, 5.0, n)[is5]
        s0 = S[SOURCE[f]]
        regime = (np.arange(n) + j) % 3
        p[:, 5] = s0 * np.choose(regime, [1.5, 0.5, 0.2])
        p[:, 6] = s0 * np.choose(regime, [3.0, 2.0, 0.6])
    if has_nan_mtt(tracer, solver):
        # pistons over the empty oldest classes for percolation and capillary rise, the uniform function for the rest; percolation
        # exceeds what leaves the subsoil's oldest class, so that class, once founded, is never clipped
        i = special["nan_mtt"]
        for f, (code, flux) in zip(FLUXES, ((1, 0.03), (1, 0.03), (2, 0.08), (1, 0.03), (2, 0.02))):
            st.sas[f][i, 0], st.sas[f][i, 1] = code, float(ages - 1)
            st.inp[f][i] = flux
    if st.anion:
        one = np.arange(n) % 3 == 0
        st.par["alpha_transp"][:] = np.where(one, 1.0, rng.uniform(0.3, 1.0, n))
        st.par["alpha_q"][:] = np.where(one, 1.0, rng.uniform(0.5, 1.0, n))
        crop = np.arange(n) % 6 == 1
        st.par["lu_id"][:] = np.where(crop, 550, 8)
        st.par["S_sat_rz"][:] = S["rz"] * np.where((np.arange(n) // 6) % 2 == 0, 0.9, 2.0)       # sum(sa) above / below 0.8 S_sat
    return st


def has_nan_mtt(tracer, solver):
    """The configurations with the NaN-marker column (special columns, above): Euler on isotopes (under RK4 a piston over an empty
    class leaves a negative trial StorAge, see the thresholds below; the anions have no marker)."""
    return solver == "Euler" and tracer in ("oxygen18", "deuterium")


def problem_of(c):
    n, ages, substeps, stats, tracer, solver = c
    return tiefree_problem(n, ages, substeps, seed_of(c), tracer=tracer, solver=solver, stats=stats)


_reference, _clip = {}, {}


def reference_days(c):
    """The oracle's NDAYS days of configuration c from the problem's start state with the same inputs every day:
    [(outputs and state after the day, margin per column)], computed once per process."""
    if c not in _reference:
        st = problem_of(c)
        days = []
        for _ in range(NDAYS):
            m = st.step_oracle(margin=True)
            _clip.setdefault(c, []).append(st.clip_margin.copy())
            snap = {k: a.copy() for k, a in st.out.items()}
            snap.update({k: a.copy() for k, a in st.state.items()})
            days.append((snap, m))
        _reference[c] = days
    return _reference[c]


def is_stat(k, a):
    """An age statistic (tt50_q_ss, rtavg_s, ..), as opposed to a distribution tt_<flux> of shape (n, ages)."""
    return k[:2] in ("tt", "rt") and np.ndim(a) == 1


def comparable(k, got_of, want_of):
    """The pair of arrays to compare for output or state array k, the project's way (sas_binding.column_deviation): the signal of an
    age class where the reference holds water (the signal of an empty class is not reproducible), mtt by its contribution mtt * tt."""
    a, b = np.asarray(got_of(k)), np.asarray(want_of(k))
    if k.startswith("msa"):
        holds = np.asarray(want_of("sa" + k[3:])) > 0
        a, b = np.where(holds, a, 0.0), np.where(holds, b, 0.0)
    if k.startswith("mtt"):
        a, b = a * got_of("tt" + k[3:]), b * want_of("tt" + k[3:])
    return a, b


def assert_columns_agree(got_of, want_of, names, keep, tag, stat_rtol=1e-9):
    """Every kept column in every array of `names`: rtol 1e-10 / atol 1e-12 (age statistics stat_rtol), NaN patterns identical.  No
    allowance."""
    for k in names:
        a, b = comparable(k, got_of, want_of)
        a, b = a[keep], b[keep]
        cols = np.flatnonzero(keep)
        nan_differs = (np.isnan(a) != np.isnan(b)).reshape(len(cols), -1).any(axis=1)
        assert not nan_differs.any(), f"{tag} {k}: NaN pattern differs in columns {cols[nan_differs][:6]}"
        ok = np.isclose(a, b, rtol=stat_rtol if is_stat(k, b) else 1e-10, atol=1e-12, equal_nan=True).reshape(len(cols), -1).all(axis=1)
        assert ok.all(), f"{tag} {k}: max dev {np.nanmax(np.abs(a - b))} in columns {cols[~ok][:6]}"


def clip_margins(c):
    """Per day the margin of configuration c without the distance of the delta values from their bounds: clips and snaps alone."""
    reference_days(c)
    return _clip[c]


def rotated_columns(c, st):
    """The unmasked columns whose SAS functions follow the rotation (the NaN-marker column has its own)."""
    keep = st.maskCatch != 0
    if has_nan_mtt(c[4], c[5]):
        keep[SPECIAL["nan_mtt"]] = False
    return keep


def rotated_variants(c, st):
    """{flux: index into variants_for(solver) of the rotated columns}."""
    keep = rotated_columns(c, st)
    return {f: variant_of(st.n, seed_of(c), len(variants_for(st.solver)))[keep, j] for j, f in enumerate(FLUXES)}
