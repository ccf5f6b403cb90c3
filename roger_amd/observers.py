"""What the device observers share on the host, once: the drain of a ring of rows, the checks of a script's request, the plumbing of
an output file, and the ordered list of the observers that `RogerSetup` walks.

An observer is a module with a class (the object on `state` a script fills in `set_diagnostics`), `initialize(state)` and, where the
device is configured later than that, `start(state)`.  The ones that record a row per step into a ring on the device derive their
class from `RingSeries` and say how rows are counted, read and written; everything about when a ring is drained is here.  The ones
that keep maps per column (scores, durations, events) derive from `Observer` and read out in their own `close`.

Restart files.  An observer whose result accumulates over the whole run (scores, durations, events, bands) names a `group` and supplies
`restart_state`; with `resume = True` on its object restart.py writes that group (`restart_groups`) and tells the observer of the file a
run continues from (`restart_read`), and the module's `start` reinstates the state (`carried_group`, `check_same_request`).  One rank
only (`check_resume`).

Adding an observer: derive its class from `RingSeries` or `Observer`, add one `Entry` to `REGISTRY`.  Nothing in roger.py changes.
"""
import collections
import datetime
import importlib
import os

import numpy as np

from . import runtime_settings as rs

DAY = 24 * 60 * 60
MAX_CELLS, MAX_VARIABLES = 256, 32     # include/roger_hip.h: rh_points_configure
WRITE_BYTES = 32 << 20                 # rows drained since the last write beyond which the file is written (as diagnostics.output)


# -- the objects on `state` --------------------------------------------------------------------------------------------------------
class Observer:
    """What every `state.<observer>` has: where its file goes, and whether the script asked for it (`active`, the same on every rank;
    `_on` is False on a rank whose block holds none of its columns)."""

    base_output_path = None
    output_path = None
    _on = False
    _path = None
    # carrying the observer's state through restart files (scores, durations, events, bands): `resume` is what a script sets, `group` the
    # restart file's group of the observer; `restart_read` notes the file a run was continued from and the group it held
    resume = False
    group = None
    _restart_file = None
    _carried = None

    def get_output_file_name(self, state):
        return output_file_name(self, state)

    def restart_state(self, state):
        """{name: array} for the observer's group of a restart file that is being written, or None (nothing to carry)."""
        return None


class RingSeries(Observer):
    """An observer whose rows the device records into a ring of `capacity` rows, one per step, and the host drains before the ring
    can wrap: after every round of device steps, every `capacity` steps of the host loops, before a restart file is written and at
    the end of run().  A subclass names itself (`label` in messages, `attribute` on state), the context it talks to, and supplies
    `_count`, `_rows` and `_write`; `_keep` where its rows are not (hdr, values) arrays."""

    label = ""                     # "points", "zonal totals", ...
    attribute = ""                 # state.<attribute>
    context = "backend_context"    # or "sas_context"
    host_header = False            # the transport rings: `stepped` notes (itt, time) of each row in _hdr, `drain` compares the counts

    def __init__(self):
        self.capacity = 4096
        self._on = False         # the device is configured (this rank holds at least one of the observer's columns)
        self._hdr = []           # drained headers (host_header: (itt, time) of every row, the ones still on the device included)
        self._values = []        # drained rows
        self._read = 0           # rows of the device's series read so far
        self._steps = 0          # host-loop steps since the last drain
        self._unwritten = 0      # bytes drained since the last write
        self._path = None

    def _begin(self):
        """The device was configured: a new series."""
        self._on, self._read, self._steps, self._unwritten = True, 0, 0, 0

    def _count(self, ctx):
        """Rows the device recorded since it was configured."""
        raise NotImplementedError

    def _rows(self, ctx, first, n):
        """(hdr, values) of the rows [first, first + n)."""
        raise NotImplementedError

    def _keep(self, state, hdr, values):
        """Hold what `_rows` gave; the bytes it takes."""
        self._hdr.append(hdr)
        self._values.append(values)
        return values.nbytes + hdr.nbytes

    def _write(self, state):
        """The whole file from the rows held in memory."""
        raise NotImplementedError

    def write(self, state):
        self._unwritten = 0
        if self._path:
            self._write(state)

    def check_call(self, nsteps):
        """Before a call that enqueues nsteps steps: a step records at most one row, more than the ring holds would overwrite rows
        nobody has read."""
        if self._on and int(nsteps) > int(self.capacity):
            raise RuntimeError(f"{int(nsteps)} steps in one call but only {int(self.capacity)} rows of the {self.label} are resident on the device: "
                               f"call run_device() in shorter pieces, or raise state.{self.attribute}.capacity")

    def drain(self, state, final=False):
        """Read the rows the device recorded since the last drain."""
        if not self._on:
            return
        ctx = getattr(state, self.context)
        total = int(self._count(ctx))
        n = total - self._read
        if n > int(self.capacity) or (self.host_header and total != len(self._hdr)):
            known = f" ({total} in all, {len(self._hdr)} steps known to the host)" if self.host_header else ""
            raise RuntimeError(f"{n} rows of the {self.label} recorded since the last drain{known} but only {int(self.capacity)} are resident on the device")
        if n > 0:
            self._unwritten += self._keep(state, *self._rows(ctx, self._read, n))
            self._read = total
        self._steps = 0
        if final or self._unwritten > WRITE_BYTES:
            self.write(state)

    def stepped(self, state):
        """A host loop made one step call: drain when the calls since the last drain reach the capacity."""
        if not self._on:
            return
        if self.host_header:
            self._hdr.append((int(state.variables.itt), int(state.variables.time)))
        self._steps += 1
        if self._steps >= int(self.capacity):
            self.drain(state)

    def close(self, state):
        """End of run(): the rest of the ring, and the file."""
        self.drain(state, final=True)


# -- the checks of a request ---------------------------------------------------------------------------------------------------------
def svat_only(what, settings, tail):
    """The refusal of an observer of the SVAT / oneD step under the offline transport model; `tail` is the observer's own sentence."""
    if settings.enable_offline_transport:
        raise NotImplementedError(f"{what}: the offline transport model steps by the day{tail}")


def check_planes(what, names, state):
    """Every name is a float64 (x, y) plane of the device arena."""
    for v in names:
        meta = state.var_meta.get(v)
        if meta is None or meta.plane is None or meta.dtype is not None:
            raise NotImplementedError(f"{what}: {v!r} is not a float64 (x, y) variable of the device arena")


def check_map_shape(what, name, a, settings):
    """A map over the global interior (`name`: "mask", "zone map", "series map") has the grid's shape."""
    if a.shape != (settings.nx, settings.ny):
        raise ValueError(f"{what}: the {name} has shape {a.shape}, the grid {settings.nx} x {settings.ny} columns")


def check_mask(what, mask, settings):
    """A mask over the global interior as booleans (None stays None): of the grid's shape, and not empty."""
    if mask is None:
        return None
    mask = np.asarray(mask)
    check_map_shape(what, "mask", mask, settings)
    mask = mask != 0
    if not mask.any():
        raise ValueError(f"{what}: the mask holds no column")
    return mask


def check_request(what, cells, n_variables, capacity, settings):
    """What the point series and the totals check alike -- the cells lie in the grid, none is given twice, the counts are within the
    recorder's limits, the ring holds a row: the cells as tuples of ints."""
    cells = [(int(c[0]), int(c[1])) for c in cells]
    for ix, iy in cells:
        if not (0 <= ix < settings.nx and 0 <= iy < settings.ny):
            raise ValueError(f"{what}: cell ({ix}, {iy}) is outside the grid of {settings.nx} x {settings.ny} columns")
    if len(set(cells)) != len(cells):
        twice = sorted({c for c in cells if cells.count(c) > 1})
        raise ValueError(f"{what}: cell {twice[0]} is given twice")
    if len(cells) > MAX_CELLS or n_variables > MAX_VARIABLES:
        raise ValueError(f"{what}: {len(cells)} cells x {n_variables} variables (at most {MAX_CELLS} x {MAX_VARIABLES})")
    if int(capacity) < 1:
        raise ValueError(f"{what}: capacity = {capacity} (at least one row resident on the device)")
    return cells


# -- resuming from a restart file ----------------------------------------------------------------------------------------------------
def check_resume(what, obs):
    """`initialize`: carrying an observer through restart files is a one-rank feature, as the output accumulators' group is."""
    from . import runtime_state

    if obs.resume and runtime_state.proc_num > 1:
        raise NotImplementedError(f"{what}: resume = True with {runtime_state.proc_num} ranks: restart files are gathered to rank 0 and the "
                                  f"observers' state is not (as for the output accumulators); set state.{what}.resume = False")


def carried_group(what, obs):
    """`start`: the observer's group of the restart file the run continues from; None for a run that does not resume (resume = False,
    or no restart file was read).  A file without the group is an error: the script asked to resume and there is nothing to resume from."""
    if not obs.resume or obs._restart_file is None:
        return None
    if obs._carried is None:
        raise RuntimeError(f"{what}: resume = True, but the restart file {obs._restart_file} holds no group {obs.group!r} (it was written "
                           f"without state.{what}.resume = True); set state.{what}.resume = False to start the observer anew from here, "
                           "as a run without resume does")
    return obs._carried


def names_array(names):
    """A list of names as bytes (restart files hold numbers only)."""
    return np.frombuffer("\n".join(str(v) for v in names).encode(), dtype=np.uint8).copy()


def map_array(a, dtype):
    """A map of a request, or an empty array for None."""
    return np.zeros(0, dtype=dtype) if a is None else np.ascontiguousarray(np.asarray(a).astype(dtype))


def _shown(key, a):
    a = np.asarray(a)
    if key in ("variables", "items"):
        return repr(bytes(a.astype(np.uint8)).decode().split("\n"))
    if a.size == 0:
        return "None"
    return repr(a.tolist()) if a.size <= 8 else f"an array of shape {a.shape}"


def request_group(request):
    """The request {key: array} as datasets of the observer's group: `request_<key>`."""
    return {f"request_{k}": np.asarray(v) for k, v in request.items()}


def check_same_request(what, obs, group, request):
    """The request of this run equals the one the restart file was written with, key by key in the request's order (NaN equals NaN)."""
    for key, want in request.items():
        want, have = np.asarray(want), group.get(f"request_{key}")
        same = have is not None and np.asarray(have).shape == want.shape and np.array_equal(
            np.asarray(have).astype(want.dtype), want, equal_nan=want.dtype.kind == "f")
        if same:
            continue
        was = "nothing" if have is None else _shown(key, have)
        where = ""
        if have is not None and np.asarray(have).shape == want.shape and want.size > 8:
            h, w = np.asarray(have).astype(want.dtype).reshape(-1), want.reshape(-1)
            differs = ~((h == w) | ((h != h) & (w != w)))
            where = f", first difference at flat index {int(np.flatnonzero(differs)[0])}"
        raise RuntimeError(f"{what}: resume = True, but the restart file {obs._restart_file} was written with {key} = {was} and this run asks "
                           f"for {key} = {_shown(key, want)}{where}: a resumed observer takes the same request")


def _block(nx, ny, num_proc, rank):
    px, py = int(num_proc[0]), int(num_proc[1])
    return int(nx) // px, int(ny) // py, rank % px, rank // px   # ranks x-fastest (distributed.proc_rank_to_index)


def local_cells(cells, nx, ny, num_proc, rank):
    """[(k, local cell)] for the points k of `cells` (global interior (ix, iy)) that lie in the block of `rank`: the local cell is
    the index rh_upload / rh_download use, C order over the rank's (x, y) interior.  Ranks x-fastest (distributed.proc_rank_to_index)."""
    nxl, nyl, bx, by = _block(nx, ny, num_proc, rank)
    return [(k, (ix - bx * nxl) * nyl + (iy - by * nyl)) for k, (ix, iy) in enumerate(cells) if ix // nxl == bx and iy // nyl == by]


def local_mask(mask, nx, ny, num_proc, rank):
    """The block of `rank` of a mask over the global interior, flat in C order over the block's (x, y).  Ranks x-fastest."""
    nxl, nyl, bx, by = _block(nx, ny, num_proc, rank)
    return np.ascontiguousarray(mask[bx * nxl:(bx + 1) * nxl, by * nyl:(by + 1) * nyl]).reshape(-1)


def interior_plane(vs, name):
    """The (x, y) interior of a variable as record 0 takes it: of a variable with time levels the one at tau."""
    a = np.asarray(getattr(vs, name))[2:-2, 2:-2]
    return a[:, :, 1] if a.ndim == 3 else a


# -- the files -----------------------------------------------------------------------------------------------------------------------
def output_file_name(series, state):
    """The file of an observer (`output_path`, `base_output_path`): one per rank, named like the diagnostics', with several ranks."""
    from . import runtime_state

    name = series.output_path.format(identifier=state.settings.identifier)
    if runtime_state.proc_num > 1:
        name = name[:-3] + f".{runtime_state.proc_rank:04d}.nc"
    return os.path.join(series.base_output_path, name) if series.base_output_path else name


def claim_output_file(series, state, what):
    """The path the observer writes to (None in diskless mode); a file that is already there is not overwritten unasked."""
    path = None if rs.diskless_mode else output_file_name(series, state)
    if path and os.path.isfile(path) and not getattr(rs, "force_overwrite", False):
        raise IOError(f"output file {path} for the {what} exists (change the output path, enable the force_overwrite runtime "
                      "setting or delete it)")
    return path


def time_variables(itt, days, time_origin, dt=None):
    """The `Time`, `dt` (where the rows have one) and `itt` variables of a file with a row per step."""
    out = {"Time": (("Time",), np.asarray(days, dtype=np.float64), {"long_name": "Time", "units": "days", "time_origin": str(time_origin)})}
    if dt is not None:
        out["dt"] = (("Time",), np.asarray(dt).astype(np.float64), {"long_name": "length of the time step", "units": "s"})
    out["itt"] = (("Time",), np.asarray(itt).astype(np.int64), {"long_name": "time step", "units": ""})
    return out


def xy_variables(vs):
    """(x, y, their variables) of this rank's block, for the files that hold maps."""
    x, y = np.asarray(vs.x)[2:-2], np.asarray(vs.y)[2:-2]
    return x, y, {"x": (("x",), x, {"long_name": "x", "units": "m"}), "y": (("y",), y, {"long_name": "y", "units": "m"})}


def global_attributes(identifier, comment, extra=None, lead=None):
    """The global attributes every file has, `lead` in front of the identifier and `extra` behind it."""
    out = {"date_created": datetime.datetime.today().isoformat(), "roger_version": "roger_amd (hip backend)", "comment": comment}
    out.update(lead or {})
    out["setup_identifier"] = str(identifier)
    out.update(extra or {})
    return out


def write_file(path, dims, variables, attributes):
    """One file through roger_amd.nc4lite, its directory made."""
    from . import nc4lite

    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    nc4lite.write(path, dims, variables, attributes)


def read_rank_files(who, paths, keys, what="variables"):
    """The front half of every `combine`: the ranks' files read, their `<name>_sum` names and the variables `keys` compared with the
    first file's.  (paths, records, names)."""
    from . import nc4lite

    paths = [str(p) for p in paths]
    if not paths:
        raise ValueError(f"{who}.combine: no files")
    recs = [nc4lite.read(p) for p in paths]
    first = recs[0]["variables"]
    names = [k[:-4] for k in first if k.endswith("_sum")]
    for p, rec in zip(paths[1:], recs[1:]):
        v = rec["variables"]
        if [k[:-4] for k in v if k.endswith("_sum")] != names:
            raise ValueError(f"{who}.combine: {p} holds other {what} than {paths[0]}")
        for key in keys:
            if not np.array_equal(np.asarray(v[key][1]), np.asarray(first[key][1])):
                raise ValueError(f"{who}.combine: {key} of {p} differs from {paths[0]}")
    return paths, recs, names


def combined_from(paths):
    return {"combined_from": ", ".join(os.path.basename(p) for p in paths)}


# -- the registry --------------------------------------------------------------------------------------------------------------------
Entry = collections.namedtuple("Entry", "attribute module cls transport ring between", defaults=(False, False, False))
"""state.<attribute> is <module>.<cls>().  transport: it observes the offline transport model (else the SVAT / oneD step).  ring: a
RingSeries.  between: not a ring, but read out between rounds of device steps and after steps of the host loops (its own `drain`
and `stepped`)."""

REGISTRY = (   # in the order of setup() and run(): it decides which error a script sees first and in which order files are claimed
    Entry("points", "points", "PointSeries", ring=True),
    Entry("totals", "totals", "AreaTotals", ring=True),
    Entry("zonal_totals", "zonal_totals", "ZonalTotals", ring=True),
    Entry("scores", "scores", "Scores"),
    Entry("events", "events", "Events", between=True),
    Entry("durations", "durations", "Durations"),
    Entry("bands", "bands", "Bands", ring=True),
    Entry("transport_points", "sas_points", "TransportPointSeries", transport=True, ring=True),
    Entry("transport_totals", "sas_totals", "TransportTotals", transport=True, ring=True),
    Entry("transport_zonal_totals", "sas_zonal_totals", "TransportZonalTotals", transport=True, ring=True),
    Entry("transport_scores", "sas_scores", "TransportScores", transport=True),
)
_RINGS = tuple(e.attribute for e in REGISTRY if e.ring)
_SVAT_RINGS = tuple(e.attribute for e in REGISTRY if e.ring and not e.transport)
# the observers a step of a host loop tells of itself, the rings first: {transport: attributes}
_PER_STEP = {t: tuple(e.attribute for e in sorted(REGISTRY, key=lambda e: not e.ring) if e.transport == t and (e.ring or e.between))
             for t in (False, True)}


def _module(entry):
    return importlib.import_module(f"{__package__}.{entry.module}")


def create(state):
    """The observers' objects on a new state."""
    for e in REGISTRY:
        setattr(state, e.attribute, getattr(_module(e), e.cls)())


def initialize(state):
    """setup(), after set_diagnostics: every observer validates what the script asked for."""
    for e in REGISTRY:
        _module(e).initialize(state)


def start(state, transport):
    """The observers that configure the device once the clock is known: those of the SVAT / oneD step after the restart file was
    read, those of the transport model when its run proper begins."""
    for e in REGISTRY:
        if e.transport == transport and hasattr(_module(e), "start"):
            _module(e).start(state)


def restart_groups(state):
    """{group: {name: array}} of the observers that carry their state through the restart file that is being written (`resume`)."""
    out = {}
    for e in REGISTRY:
        o = getattr(state, e.attribute)
        held = o.restart_state(state) if o.resume and o.group else None
        if held:
            out[o.group] = held
    return out


def restart_read(state, fname, groups):
    """A restart file was read: every observer learns of it and of its own group in it; `start` takes it from there."""
    for e in REGISTRY:
        o = getattr(state, e.attribute)
        o._restart_file, o._carried = fname, (groups.get(o.group) if o.group else None)


def check_call(state, nsteps):
    """Before run_device enqueues nsteps steps."""
    for a in _SVAT_RINGS:
        getattr(state, a).check_call(nsteps)


def drain_rings(state, final=False):
    """Every ring: the rows not yet read (before a restart file is written, around a round of device steps)."""
    for a in _RINGS:
        getattr(state, a).drain(state, final=final)


def drain_round(state, final=False):
    """After a round of device steps: the rings, then what else is read out between rounds."""
    for a in _PER_STEP[False]:
        getattr(state, a).drain(state, final=final)


def stepped(state, transport=False):
    """A host loop made one step."""
    for a in _PER_STEP[transport]:
        getattr(state, a).stepped(state)


def needs_end_of_step(state):
    """Does any observer the script asked for look at every step of the host loops of the SVAT / oneD model?"""
    return any(getattr(state, a).active for a in _PER_STEP[False])


def ring_capacity(state):
    """The smallest capacity over the rings the script asked for (`active`: the same on every rank, so a collective round has one
    length), None without any: a round of device steps never records more rows than a ring holds."""
    asked = [int(getattr(state, a).capacity) for a in _SVAT_RINGS if getattr(state, a).active]
    return min(asked) if asked else None


def close(state):
    """End of run(): the rest of every ring, the maps, the files."""
    for e in REGISTRY:
        getattr(state, e.attribute).close(state)
