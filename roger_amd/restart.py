"""Checkpoint / restart of a model state on the hip backend: roger/restart.py's `write_restart` / `read_restart` in the reference's
file layout -- an HDF5 file whose group "core" holds one dataset per variable under the variable's name, in the reference's GLOBAL
array shape (2-cell ghost frame included, trailing `timesteps` axis for the two-level variables, 0-d datasets for the scalars;
roger/restart.py:32-67, 129-174), so that states can go back and forth between the two implementations.

* What is written: group "core" = every `write_to_restart` variable of the reference that this path holds
  (`REFERENCE_RESTART_VARIABLES`, read off roger/variables.py) and nothing else -- the reference's reader walks every dataset of
  "core" and fails on a name that is not on its list (roger/restart.py:15-16); group "hip_core" = every other variable of the arena:
  the reference's own list does not carry the whole state of a step (`prec`, `ta`, the event bookkeeping of the wetting fronts ... are
  missing from it), with the rest of the planes a restarted run continues BIT FOR BIT (tests/test_hip_restart.py).  Exchanged with
  the reference in both directions: tests/test_restart_interchange.py.
* The device-side output accumulators (rh_diag_*) go into the group "hip_diag": a restart in the middle of an output interval keeps
  the partial sums.
* The observers that accumulate over the whole run -- state.scores, state.durations, state.events, state.bands -- go, where the script
  sets `state.<observer>.resume = True`, into the groups "hip_scores", "hip_durations", "hip_events", "hip_bands": their device state
  and the few host numbers that reinstate it (Observer.restart_state / the modules' `start`, walked over observers.REGISTRY: this module
  names no observer).  The reference's reader opens "core" and the groups of its own diagnostics and nothing else, so these groups, like
  "hip_core" and "hip_diag", leave the file readable for it.  One rank only, as "hip_diag".  Without `resume` nothing is written.
* Several ranks (num_proc = (px, py)): the blocks are gathered to rank 0, which writes ONE file with the global arrays like the
  reference's MPI-IO write (roger/restart.py:43-64); every rank reads its own chunk, ghost frame included (`get_chunk_slices(...,
  include_overlap=True)`, :20-24).
* Container: h5py where it is installed; otherwise `roger_amd.h5lite`, a small classic-HDF5 writer / reader (contiguous datasets;
  it reads the chunked + gzip files h5py writes for the reference).

Driven like the reference: `settings.restart_input_filename` is read at the end of `setup()` (roger/roger.py:324-326),
`settings.restart_output_filename` (Python format syntax over the variables and settings, :156-158) is written every
`settings.restart_frequency` seconds at the start of a step (:385-386) and, with `settings.write_restart`, at the end of `run()`
(:578-579); `runtime_settings.diskless_mode` suppresses writing (:134).

Offline transport (settings.enable_offline_transport, the SAS model) -- same settings, same groups, its own contents:
* "core": the names of `REFERENCE_RESTART_VARIABLES` the transport registry has (the grid, the clock, the storages of the SVAT run it
  reads); "hip_core": the rest of what the next day step reads -- the per-cell variables of the SAS context (concentrations, solute
  masses, age statistics, parameters) and of the host (the snow signal and the other time levels the hooks read back), `ages` /
  `nages`, `warmup_done` (0-d) and the tracer / solver codes of the run (`sas_tracer`: index in `_TRACERS`, `sas_solver`:
  _native.SAS_SOLVERS), against which `read_restart` checks the model -- and the age-resolved storages sa_rz, sa_ss, msa_rz, msa_ss, sa_s,
  msa_s as (nx, ny, ages) datasets: the interior of time level tau, the only level the device holds (both levels agree after a step).
* Left out: the forcing series (x, y, t) that set_forcing_setup rebuilds (PREC_DIST_DAILY, INF_*, C_IN, C_ISO_IN ...), the
  distributions tt_*, mtt_*, TT_* (every step rewrites them before anything reads them) and the host-side age diagnostics SA_*,
  csa_* (set by the script's initial conditions, never touched by the step): at 10^6 columns x 1000 ages each of these is 8 GB.
* The age-resolved storages never exist on the host in full: they are streamed between the SAS context and the file in blocks of
  `BLOCK_BYTES` (rh_sas_download_cells / rh_sas_upload_cells), so a write holds one block of them at a time.  Several ranks: rank 0
  writes the file; the other ranks send their blocks to it one at a time over the process group (torch.distributed send / recv), so
  no rank holds more than a block either (verified over gloo; the send / recv of device tensors under NCCL / RCCL is not tested).  Each
  rank reads its own cells back.  Nothing on the write path reads an age-resolved `vs.<name>`: that would download the whole array
  into its host mirror (`_restart_filename` picks the scalars by their metadata for that reason).
* Container: h5py where it is installed, otherwise h5lite's block-wise writer / reader (`h5lite.create`, `h5lite.open_blocks`).
* Not claimed: that the reference's reader accepts a transport file.  No restart file of the reference's transport models is
  available to check against; what is checked is that an interrupted run continues bit for bit
  (tests/test_host_package_sas_restart.py, tests/test_hip_sas_restart.py)."""
import os

import numpy as np

from . import distributed, h5lite, logger, observers, runtime_settings as rs, runtime_state as rst

# roger/variables.py: the variables with write_to_restart=True that exist on this path (the others belong to modules that are out of
# scope: crops, film flow, groundwater, routing, transport)
REFERENCE_RESTART_VARIABLES = (
    "maskCatch", "maskRiver", "maskLake", "lu_id", "sealing", "z0", "slope", "slope_per", "S_dep_tot", "ground_cover", "lai",
    "throughfall_coeff_top", "throughfall_coeff_ground", "basal_evap_coeff", "k_stress_evap", "evap_coeff", "basal_transp_coeff",
    "k_stress_transp", "transp_coeff", "S_int_top_tot", "S_int_ground_tot", "S", "S_snow", "swe", "swe_top", "swe_top_tot", "swe_ground",
    "S_dep", "S_sur", "S_int_top", "S_int_ground", "z_soil", "c_root", "clay", "sand", "lmpv", "lmpv_non_sat", "z_sc", "z_sc_non_sat",
    "dmpv", "mp_drain_area", "dmph", "theta_ufc", "theta_ac", "theta_pwp", "theta_sat", "theta_fc", "theta_27", "theta_4", "theta_6",
    "S_ufc_s", "S_ac_s", "S_pwp_s", "S_sat_s", "S_fc_s", "wfs", "ks", "ks_ss", "ha", "lambda_bc", "m_bc", "n_salv", "z_sc_max", "kf",
    "theta", "theta_d", "theta_d_fp", "theta_d_rel", "theta_d_rel_t0", "theta_d_t0", "theta_d_t1", "S_s", "S_fp_s", "S_lp_s", "S_zsat",
    "k", "h", "y_mp", "y_sc", "z_wf", "z_wf_t0", "z_wf_t1", "z_wf_fc", "z_sat_layer_1", "z_sat_layer_2", "z_sat_layer_3", "z_sat_layer_4",
    "z_sat_layer_5", "z_sat_layer_6", "z_sat_layer_7", "z_sat_layer_8", "z_sat", "z_root", "z_evap", "tew", "rew", "de", "k_rz", "h_rz",
    "theta_rz", "theta_fp_rz", "theta_lp_rz", "S_rz", "S_fp_rz", "S_lp_rz", "S_pwp_rz", "S_fc_rz", "S_sat_rz", "S_ufc_rz", "S_ac_rz",
    "k_ss", "h_ss", "theta_ss", "theta_fp_ss", "theta_lp_ss", "S_ss", "S_fp_ss", "S_lp_ss", "S_zsat_ss", "S_pwp_ss", "S_fc_ss",
    "S_sat_ss", "S_ufc_ss", "S_ac_ss", "z_gw", "no_wf", "pi_gr", "pi_m", "t_sat", "Fs", "Fs_t0", "inf_mat_pot_event_csum",
    "inf_mat_event_csum", "inf_mp_event_csum", "inf_sc_event_csum", "evap_int", "prec_event_csum", "t_event_csum", "c_int",
    # scalars (0-d datasets)
    "time", "time_event0", "itt", "itt_day", "itt_forc", "year", "month", "doy", "dt", "dt_secs", "event_id", "event_id_counter",
    # the forcing series and the grid (the reference restarts them too)
    "PREC", "TA", "PET", "YEAR", "MONTH", "DOY", "x", "y",
)
# ... and the rest of the reference's list for these models: variables of modules outside this path (crops, film flow, radiation) and
# registry constants.  The reference's reader insists on finding EVERY variable of its list (roger/restart.py:93-97), so a file that
# the reference is to accept carries them with the values the reference itself writes for an SVAT / oneD run: its initial values
# (read off a restart file of the reference, tests/golden/restart/reference_restart.h5).  name: (dims, dtype, value)
REFERENCE_ONLY_RESTART_VARIABLES = {
    **{k: (("x", "y"), "float64", 0.0) for k in (
        "Fs_t1", "c1_mak", "c2_mak", "dmpv_crop", "frac_fp", "frac_lp", "lmpv_crop", "t_sat_t0", "t_sat_t1", "theta_ac_ss", "theta_d_rel_t1",
        "theta_eff", "theta_fp", "theta_lp", "theta_pc", "theta_water_stress", "water_stress_fp")},
    "zroot_to_zsoil_max": (("x", "y"), "float64", 0.75),
    "maskUrban": (("x", "y"), "bool", 0),
    "RS": (("t_forc",), "float64", 0.0),
    **{k: ((), "int64", v) for k, v in dict(itt_cr=0, itt_substep=0, tau=1, taum1=0, taup1=2, tau_event=0, time_for_diag=86400).items()},
    "z": (("z",), "float64", 0.0),
}
# on the reference's list only with settings.enable_lateral_flow (oneD model)
_LATERAL_ONLY = ("dmph",) + tuple(f"z_sat_layer_{i}" for i in range(1, 9))
_NOT_STATE = ("tau", "taup1", "taum1")   # constants of the registry
MORE_GROUP = "hip_core"   # the variables of the arena that are not on the reference's restart list
# inputs that set_forcing_setup puts back at setup(), not state: the station series and the calendar (at 10^6 columns the series of a
# distributed setup and the per-cell day arrays below are gigabytes)
_FORCING_SERIES = ("PREC_DIST", "TA_DIST", "PET_DIST")   # (the single station's series are on the reference's own list: kept)
# the day's 144 slots per cell: set_forcing re-derives them from itt_forc at midnight, so they are state only in the middle of a day
_FORCING_DAY = ("prec_day", "ta_day", "pet_day")


def _h5py():
    try:
        import h5py

        return h5py
    except ImportError:
        return None


def _write_file(path, groups):
    h5py = _h5py()
    if h5py is None:
        return h5lite.write(path, groups)
    with h5py.File(path, "w") as f:
        for gname, dsets in groups.items():
            g = f.require_group(gname)
            for k, a in dsets.items():
                a = np.asarray(a)
                g.create_dataset(k, data=a.astype(np.int8) if a.dtype == np.bool_ else a)


def _read_file(path):
    h5py = _h5py()
    if h5py is None:
        return h5lite.read(path)
    with h5py.File(path, "r") as f:
        return {gname: {k: np.asarray(v) for k, v in g.items()} for gname, g in f.items()}


def _restart_filename(state, template):
    """The template formatted with the scalars and the settings.  The scalars are picked by their metadata (no dims): an array is never
    read here -- for the transport model that would download every age-resolved variable a step left newer on the device."""
    statedict = {}
    for key, var in state.var_meta.items():
        if var.dims is not None:
            continue
        try:
            v = np.asarray(getattr(state.variables, key))
        except Exception:   # noqa: BLE001
            continue
        if v.ndim == 0:
            statedict[key] = v.item()
    statedict.update({k: getattr(state.settings, k) for k in state.settings.__metadata__})
    return template.format(**statedict)


def _gather_global(state, key, local):
    """The global array (ghost frame included) of an (x, y, ...) variable from the ranks' slabs, on rank 0; None elsewhere."""
    import torch.distributed as dist

    world, rank = rst.proc_num, rst.proc_rank
    parts = [None] * world if rank == 0 else None
    dist.gather_object(np.asarray(local), parts, dst=0)
    if rank != 0:
        return None
    nx, ny = state.settings.nx, state.settings.ny
    out = np.zeros((nx + 4, ny + 4) + local.shape[2:], dtype=local.dtype)
    for r, part in enumerate(parts):
        (gx, gy), (lx, ly) = distributed.get_chunk_slices(nx, ny, rs.num_proc, r, include_overlap=True)
        out[gx, gy] = part[lx, ly]
    return out


def collect(state):
    """{group: {name: array}} of everything a restart file holds."""
    vs = state.variables
    core = {}
    multi = rst.proc_num > 1
    # The day's 3 x (x, y, 144) forcing arrays are left out at midnight ONLY where the script's set_forcing is known to re-derive them
    # there (the stock hook, or one recognised as doing the same: roger_amd/hooks.py); a set_forcing of the script's own that does
    # not must find the arrays it left.
    midnight = int(np.asarray(vs.time)) % 86400 == 0 and state._stock_set_forcing
    more = {}
    for key, var in state.var_meta.items():
        if key in _NOT_STATE or key in _FORCING_SERIES or (midnight and key in _FORCING_DAY):
            continue
        val = np.asarray(getattr(vs, key))
        if multi and var.dims is not None and tuple(var.dims[:2]) == ("x", "y"):
            val = _gather_global(state, key, val)
        # the reference's reader walks EVERY dataset of "core" and looks it up in its own restart list (roger/restart.py:15-16:
        # a KeyError for anything else), so "core" holds exactly that list; the rest of the arena goes into a group of its own,
        # which the reference never opens
        on_list = key in REFERENCE_RESTART_VARIABLES and (state.settings.enable_lateral_flow or key not in _LATERAL_ONLY)
        (core if on_list else more)[key] = val
    sizes = dict(x=state.settings.nx + 4, y=state.settings.ny + 4, t_forc=state.settings.nitt_forc, z=1)
    for key, (dims, dtype, value) in REFERENCE_ONLY_RESTART_VARIABLES.items():
        core.setdefault(key, np.full(tuple(sizes[d] for d in dims), value, dtype=dtype))
    groups = {"core": core, MORE_GROUP: more}
    # one group per diagnostic of the reference that has restart variables (roger/restart.py:100-126 opens every one of them): the
    # counters of the monitors and of the average diagnostic, as the reference writes them when those diagnostics are not in use
    groups.update({"average": {"average_nitts": np.float64(0.0)}, "snapshot": {},
                   "tracer_monitor": {"C_s": np.float64(0.0), "M_S": np.float64(0.0)},
                   "water_monitor": {"S_s": np.float64(0.0), "S_sur": np.float64(0.0)}})
    ctx = state.backend_context
    active = state._diag_active
    if active and not state._diag_transport and not multi:
        # the accumulators of the output interval the run is in (roger_amd/diagnostics.py; completed intervals were written out)
        iv = state._diag_interval
        slot = int(int(np.asarray(vs.time)) // iv) % state._diag_slots
        names = list(dict.fromkeys(v for d in active for v in d.output_variables))
        t0, t1 = ctx.diag_slot_times(slot)
        groups["hip_diag"] = {nm: ctx.diag_download(nm, slot) for nm in names}
        groups["hip_diag"]["slot_state"] = np.array([slot, ctx.diag_steps(slot), t0, t1, state._diag_written_day], dtype=np.int64)
    # the observers a script set `resume` on: one group each ("hip_scores", "hip_durations", "hip_events", "hip_bands"), next to the two
    # above and like them never opened by the reference's reader; nothing without `resume` (roger_amd/observers.py: restart_groups)
    groups.update(observers.restart_groups(state))
    return groups


# ---- offline transport ----------------------------------------------------------------------------------------------------------------
AGE_STATE = ("sa_rz", "sa_ss", "msa_rz", "msa_ss", "sa_s", "msa_s")   # streamed (nx, ny, ages) datasets
BLOCK_BYTES = 64 << 20   # age-resolved data per block of columns (upload / download / file / process group)
_TRACERS = ("oxygen18", "deuterium", "bromide", "chloride", "virtualtracer")   # the codes of `sas_tracer` in a file


def _transport_small(state):
    """{group: {name: array}} of everything but the age-resolved storages (global arrays on rank 0, None on the other ranks)."""
    vs, settings = state.variables, state.settings
    multi = rst.proc_num > 1
    core, more = {}, {}
    for key, var in state.var_meta.items():
        dims = tuple(var.dims or ())
        if key in _NOT_STATE or key in AGE_STATE or "t" in dims or (dims[:2] == ("x", "y") and ("ages" in dims or "nages" in dims)):
            continue
        if var.sas is not None and not _held(state.sas_context, var.sas):
            continue   # (a variable of the registry whose array this tracer's context does not allocate, e.g. M_evap_soil)
        val = np.asarray(getattr(vs, key))
        if multi and dims[:2] == ("x", "y"):
            val = _gather_global(state, key, val)
        elif multi and dims in (("x",), ("y",)):
            val = _gather_coordinate(state, key, val)
        (core if key in REFERENCE_RESTART_VARIABLES else more)[key] = val
    from . import _native

    more["warmup_done"] = np.array(int(bool(settings.warmup_done)), dtype=np.int64)
    more["sas_tracer"] = np.array(_TRACERS.index(state.sas_context.tracer), dtype=np.int64)
    more["sas_solver"] = np.array(_native.SAS_SOLVERS[state.sas_context.solver], dtype=np.int64)
    return {"core": core, MORE_GROUP: more}


def _held(sas, name):
    try:
        sas.shape(name)
    except (KeyError, RuntimeError):
        return False
    return True


def _block_cells(sas):
    return max(1, BLOCK_BYTES // (8 * sas.ages))


def _row_runs(nx, ny, rank, first, count):
    """The runs of cells [first, first + count) of a rank's block (C order over its (nxl, nyl) cells) along the global grid's rows:
    (offset in the block, global x, global y of the run's first cell, length)."""
    (gx, gy), _ = distributed.get_chunk_slices(nx, ny, rs.num_proc, rank)
    nyl = gy.stop - gy.start
    c = first
    while c < first + count:
        i, j = divmod(c, nyl)
        n = min(nyl - j, first + count - c)
        yield c - first, gx.start + i, gy.start + j, n
        c += n


def _p2p_device():
    """Where point-to-point blocks travel from: host memory over gloo, the rank's device over NCCL / RCCL.  Only the gloo path is
    exercised by the tests (tests/test_host_package_sas_restart.py, two CPU ranks); the NCCL / RCCL path is not verified."""
    import torch
    import torch.distributed as dist

    return torch.device("cuda", torch.cuda.current_device()) if dist.get_backend() == "nccl" else torch.device("cpu")


def _gather_coordinate(state, key, local):
    """The global (x,) / (y,) coordinate of a grid split over several ranks, on rank 0; None elsewhere."""
    import torch.distributed as dist

    world, rank = rst.proc_num, rst.proc_rank
    parts = [None] * world if rank == 0 else None
    dist.gather_object(np.asarray(local), parts, dst=0)
    if rank != 0:
        return None
    axis = state.var_meta[key].dims[0]
    nx, ny = state.settings.nx, state.settings.ny
    out = np.zeros((nx if axis == "x" else ny) + 4, dtype=local.dtype)
    for r, part in enumerate(parts):
        g, l = distributed.get_chunk_slices(nx, ny, rs.num_proc, r, include_overlap=True)
        k = 0 if axis == "x" else 1
        out[g[k]] = part[l[k]]
    return out


class _H5pyBlocks:
    """The block-wise file of `_write_transport` / `_read_transport` over h5py."""

    def __init__(self, path, groups, mode):
        import h5py

        self.f = h5py.File(path, mode)
        if mode == "w":
            for gname, dsets in groups.items():
                g = self.f.require_group(gname)
                for k, a in dsets.items():
                    if isinstance(a, h5lite.Deferred):
                        g.create_dataset(k, shape=a.shape, dtype=a.dtype)
                    else:
                        a = np.asarray(a)
                        g.create_dataset(k, data=a.astype(np.int8) if a.dtype == np.bool_ else a)

    def has(self, group, name):
        return group in self.f and name in self.f[group]

    def shape(self, group, name):
        return self.f[group][name].shape

    def put_row(self, group, name, x, y, rows):
        self.f[group][name][x, y:y + len(rows)] = rows

    def get_row(self, group, name, x, y, n):
        return self.f[group][name][x, y:y + n]

    def close(self):
        self.f.close()


class _LiteBlocks:
    """The same over h5lite's StreamFile (contiguous (nx, ny, ages) datasets: a row run is one contiguous range)."""

    def __init__(self, stream):
        self.s = stream

    def has(self, group, name):
        return (group, name) in self.s._where

    def shape(self, group, name):
        return self.s.shape(group, name)

    def put_row(self, group, name, x, y, rows):
        nx, ny, ages = self.s.shape(group, name)
        self.s.put(group, name, (x * ny + y) * ages, rows)

    def get_row(self, group, name, x, y, n):
        nx, ny, ages = self.s.shape(group, name)
        return self.s.get(group, name, (x * ny + y) * ages, n * ages).reshape(n, ages)

    def close(self):
        self.s.close()


def _write_transport(state, fname):
    import torch
    import torch.distributed as dist

    vs, settings, sas = state.variables, state.settings, state.sas_context
    vs.flush_to_device()
    groups = _transport_small(state)
    rank, world = rst.proc_rank, rst.proc_num
    names = [k for k in AGE_STATE if k in state.var_meta]
    out = None
    if rank == 0:
        logger.info(f"Writing restart file {fname}")
        for k in names:
            groups[MORE_GROUP][k] = h5lite.Deferred((settings.nx, settings.ny, sas.ages), np.float64)
        out = _H5pyBlocks(fname, groups, "w") if _h5py() is not None else _LiteBlocks(h5lite.create(fname, groups))
    step = _block_cells(sas)
    dev = _p2p_device() if world > 1 else None
    try:
        for k in names:
            for first in range(0, sas.n, step):   # (every rank holds the same number of cells: the blocks line up)
                count = min(step, sas.n - first)
                block = sas.download_cells(k, first, count)
                if rank != 0:
                    dist.send(torch.from_numpy(block).to(dev), dst=0)
                    continue
                for r in range(world):
                    if r:
                        t = torch.empty(block.shape, dtype=torch.float64, device=dev)
                        dist.recv(t, src=r)
                        block = t.cpu().numpy()
                    for off, x, y, n in _row_runs(settings.nx, settings.ny, r, first, count):
                        out.put_row(MORE_GROUP, k, x, y, block[off:off + n])
    finally:
        if out is not None:
            out.close()


def _read_transport(state, fname):
    """The transport branch of `read_restart`: checks the file against the model, assigns the small variables, streams the age-resolved
    storages of this rank's cells into the SAS context."""
    from . import _native

    vs, settings, sas = state.variables, state.settings, state.sas_context
    if _h5py() is not None:
        blocks = _H5pyBlocks(fname, None, "r")
        small = {g: {k: np.asarray(v) for k, v in grp.items() if k not in AGE_STATE} for g, grp in blocks.f.items()}
    else:
        small, stream = h5lite.open_blocks(fname, streamed=AGE_STATE)
        blocks = _LiteBlocks(stream)
    try:
        more = small.get(MORE_GROUP, {})
        if "sas_tracer" not in more or not blocks.has(MORE_GROUP, "sa_rz"):
            raise RuntimeError(f"{fname} is not a restart file of the offline transport model")
        want = dict(sas_tracer=_TRACERS.index(sas.tracer), sas_solver=_native.SAS_SOLVERS[sas.solver])
        for k, v in want.items():
            if int(more[k]) != v:
                raise RuntimeError(f"{fname} was written with {k} = {int(more[k])}, the model has {v} ({sas.tracer}, {sas.solver})")
        shape = tuple(blocks.shape(MORE_GROUP, "sa_rz"))
        if shape[:2] != (settings.nx, settings.ny):
            raise RuntimeError(f"{fname} holds a {shape[0]} x {shape[1]} grid, the model has {settings.nx} x {settings.ny}")
        if shape[2] != settings.ages or np.asarray(more.get("ages", ())).shape != (settings.ages,) or \
                np.asarray(more.get("nages", ())).shape != (settings.nages,):
            raise RuntimeError(f"{fname} holds {shape[2]} age classes, the model has settings.ages = {settings.ages}")
        vs.flush_to_device()   # (what setup() assigned must not overwrite the streamed storages at the next native call)
        nx, ny = settings.nx, settings.ny
        (gx, gy), (lx, ly) = distributed.get_chunk_slices(nx, ny, rs.num_proc, rst.proc_rank, include_overlap=True)
        with vs.unlock():
            for gname in ("core", MORE_GROUP):
                for key, val in small.get(gname, {}).items():
                    if key not in state.var_meta or key in _NOT_STATE:
                        continue
                    var = state.var_meta[key]
                    val = np.asarray(val)
                    if var.dims is None:
                        setattr(vs, key, val.item())
                        continue
                    if rst.proc_num > 1 and tuple(var.dims[:2]) == ("x", "y"):
                        local = np.array(getattr(vs, key))
                        local[lx, ly] = val[gx, gy]
                        val = local
                    elif rst.proc_num > 1 and tuple(var.dims) in (("x",), ("y",)):
                        g, l = (gx, lx) if var.dims[0] == "x" else (gy, ly)
                        local = np.array(getattr(vs, key))
                        local[l] = val[g]
                        val = local
                    setattr(vs, key, val.astype(np.asarray(getattr(vs, key)).dtype))
        with settings.unlock():
            settings.warmup_done = bool(int(more["warmup_done"]))
        vs.flush_to_device()
        step = _block_cells(sas)
        buf = np.empty((min(step, sas.n), sas.ages))
        for k in (k for k in AGE_STATE if k in state.var_meta):
            for first in range(0, sas.n, step):
                count = min(step, sas.n - first)
                for off, x, y, n in _row_runs(nx, ny, rst.proc_rank, first, count):
                    buf[off:off + n] = blocks.get_row(MORE_GROUP, k, x, y, n)
                sas.upload_cells(k, first, buf[:count])
        vs.mark_device_newer([k for k in AGE_STATE if k in state.var_meta])
    finally:
        blocks.close()


def write_restart(state, force=False, filename=None):
    """roger/restart.py:129-174.  Returns the file name (None if nothing was due)."""
    vs, settings = state.variables, state.settings
    if rs.diskless_mode and filename is None:
        return None
    template = filename or settings.restart_output_filename
    if not template:
        return None
    write_now = force or filename is not None or (
        settings.restart_frequency > 0 and int(np.asarray(vs.itt)) > 0 and int(np.asarray(vs.time)) % settings.restart_frequency == 0)
    if not write_now:
        return None
    fname = _restart_filename(state, str(template))
    if state.settings.enable_offline_transport:
        _write_transport(state, fname)
        return fname
    groups = collect(state)
    if rst.proc_rank == 0:
        logger.info(f"Writing restart file {fname}")
        _write_file(fname, groups)
    return fname


def read_restart(state, filename=None):
    """roger/restart.py:70-126: assigns every variable found in the group "core" (shape- and dtype-checked by RogerVariables like any
    assignment); the device copies are refreshed before the next native call."""
    settings = state.settings
    template = filename or settings.restart_input_filename
    if not template:
        return None
    if rs.force_overwrite:
        raise RuntimeError("To prevent data loss, force_overwrite cannot be used in restart runs")
    fname = _restart_filename(state, str(template))
    if not os.path.isfile(fname):
        raise IOError(f"restart file {fname} not found")
    logger.info(f"Reading restart data from {fname}")
    if settings.enable_offline_transport:
        _read_transport(state, fname)
        return fname
    groups = _read_file(fname)
    if "core" not in groups:
        raise RuntimeError(f"{fname} has no group 'core': not a RoGeR restart file")
    core = dict(groups["core"])
    core.update(groups.get(MORE_GROUP, {}))   # a file of the reference has "core" only: the rest keeps what setup() left
    vs = state.variables
    missing = [k for k in REFERENCE_RESTART_VARIABLES if k in state.var_meta and k not in core and k not in ("dmph",) + tuple(
        f"z_sat_layer_{i}" for i in range(1, 9)) + ("slope", "slope_per")]
    if missing:
        raise RuntimeError(f"No restart data found for variable {missing[0]} in {fname}")
    nx, ny = settings.nx, settings.ny
    (gx, gy), (lx, ly) = distributed.get_chunk_slices(nx, ny, rs.num_proc, rst.proc_rank, include_overlap=True)
    with vs.unlock():
        for key, val in core.items():
            if key not in state.var_meta or key in _NOT_STATE:
                continue   # a variable of a module this path does not have
            var = state.var_meta[key]
            val = np.asarray(val)
            if var.dims is None:
                setattr(vs, key, val.item() if val.ndim == 0 else val)
                continue
            if tuple(var.dims[:2]) == ("x", "y") and rst.proc_num > 1:
                local = np.array(getattr(vs, key))
                local[lx, ly] = val[gx, gy]
                val = local
            if np.asarray(getattr(vs, key)).dtype == np.bool_:
                val = val.astype(np.bool_)
            setattr(vs, key, val)
    active = state._diag_active
    if active and "hip_diag" in groups and rst.proc_num == 1 and not state._diag_transport:
        ctx = state.backend_context
        slot, steps, t0, t1, written = (int(v) for v in groups["hip_diag"]["slot_state"])
        for nm in dict.fromkeys(v for d in active for v in d.output_variables):
            if nm in groups["hip_diag"]:
                ctx.diag_upload(nm, slot, groups["hip_diag"][nm])
        ctx.diag_set_slot_state(slot, steps, t0, t1)
        state._diag_written_day = written
    observers.restart_read(state, fname, groups)   # (their `start` follows: roger.py)
    return fname
