"""The coupling time loop of the reference main program (flux_calculator.F90:859-1026,
STEP 2) for a Python host, on a set-up from fcx.setup and an fcx.Engine.

Per coupling step, in the reference order:
  2.1  oasis_get of the early received fields (grids t, u, v; list order), then
       do_regridding of each early received field (F90:874-897);
  2.2  the early calculations: RBBR and its regridding           -> engine phase EARLY;
  2.3  oasis_put of the early sent fields, each type-0 field averaged first when the
       put loop's trigger holds (F90:906-937)                    -> averages in phase EARLY;
  2.4  oasis_get of the normal received fields + their regridding (F90:943-958);
  2.5  QSUR, MEVA, HLAT, HSEN, UMOM, VMOM with their regriddings, the shortwave
       distribution (F90:964-988)                                -> engine phase NORMAL;
  2.6  oasis_put of the normal sent fields, averaged first as in 2.3 (F90:994-1022).
The coupler stands in for OASIS3-MCT: `get(name, time, out)` fills the received field's
array in place (oasis_get writes through the io_field pointer), `put(name, time, array)`
takes the sent field.  The engine's step(phase) uploads what the phase reads, runs it on
the GPU and downloads what it writes, so the arrays the coupler sees are the host
local_field arrays exactly as in the reference loop.  A field the set-up receives on its
model's grid (FluxCalculatorSetup.engine(receive_maps=...)) is the exception: the coupler
fills setup.source_field[name], and the engine expands it on the device.
"""
from .basic import PHASE_EARLY, PHASE_NORMAL


def _regridded(lf, f):
    """Does do_regridding(f.var, f.surface_type) have any put_to flag to act on?"""
    types = range(1, 11) if f.surface_type == 0 else (f.surface_type,)
    return any(lf.put_to.get((s, g, f.var), 0) for s in types for g in (1, 2, 3))


VERBOSITY_LEVEL_DEBUG = 2  # flux_calculator_basic.F90:70-72


def _log_ranges(setup, engine, early, current_time, log):
    """The reference's DEBUG lines of a phase (flux_calculator.F90:879-881, 921-924, 949-951,
    1011-1013): name, MINVAL, MAXVAL of every received and every sent field.  ONE fcx_field_ranges
    call covers everything the device holds -- so a field received on its model's grid reports
    the exchange-grid array the calculation saw, and an output kept on the device is reported at
    all; host arrays the host filled itself are reduced where they are."""
    import numpy as np

    lf = setup.local_field
    sources = getattr(setup, "source_field", {})
    computed = {id(lf.field[s]) for s in setup.computed_slots() if s in lf.field}
    fields = [("received", f) for f in setup.fields_in_put_order(setup.input_field, early)]
    fields += [("sent", f) for f in setup.fields_in_put_order(setup.output_field, early)]

    def on_device(what, f):
        # what only the device holds, or holds as the step left it: a field gathered from its
        # model grid, a computed output, any array resident in device memory.  A host array the
        # host itself filled (a received field, a default-valued send) is the value as it is: the
        # engine uploads only what a calculation reads.
        a = lf.field[f.slot]
        return not isinstance(a, np.ndarray) or (f.name in sources if what == "received" else id(a) in computed)

    asked = [f.slot for what, f in fields if on_device(what, f)]
    ranges = iter(engine.field_ranges(asked) if asked else ())
    for what, f in fields:
        if on_device(what, f):
            r = next(ranges)
            lo, hi = r.min, r.max
        else:
            a = lf.field[f.slot][: lf.grid_size[f.which_grid - 1]]
            lo, hi = (float(np.fmin.reduce(a)), float(np.fmax.reduce(a))) if a.size else (float("nan"),) * 2
        log(f"  {what}  {f.name} at runtime={current_time} seconds: range = {lo!r} {hi!r}")


def _log_budgets(setup, engine, early, phase, current_time, budgets):
    """A phase's flux budgets: name and area-weighted integral of every sent field, exact on the
    device (ONE fcx_field_integrals call; the engine needs the grids' areas, Engine.set_areas).
    Where the engine accumulates the field onto the atmosphere grid and holds the atmosphere
    cells' areas (Engine.set_atmos_areas), the line also gives the atmosphere-side integral and
    the difference of the two exact sums, rounded once: what the step failed to conserve."""
    sent = setup.fields_in_put_order(setup.output_field, early)
    if not sent:
        return
    sums = list(engine.field_integrals([f.slot for f in sent]))
    twins = engine.atmos_twins(phase)
    atmo = dict(zip(twins, engine.atmos_integrals(phase))) if twins else {}
    for f, sx in zip(sent, sums):
        line = f"  budget  {f.name} at runtime={current_time} seconds: integral = {sx.value!r}"
        sa = atmo.get(tuple(f.slot))
        if sa is not None:
            line += f" atmosphere = {sa.value!r} difference = {(sx + (-sa)).value!r}"
        budgets(line)


def coupling_step(setup, engine, coupler, current_time, log=None, budgets=None):
    """log: a callable taking one line; with nml["verbosity_level"] at DEBUG every phase then
    reports the ranges of its received and sent fields (_log_ranges).  None: no range call.
    budgets: a callable taking one line; every phase then reports the area-weighted integral of
    each sent field after its step (_log_budgets).  None: no integral call."""
    lf = setup.local_field
    debug = log is not None and setup.nml.get("verbosity_level", 1) >= VERBOSITY_LEVEL_DEBUG
    for early, phase in ((True, PHASE_EARLY), (False, PHASE_NORMAL)):
        sources = getattr(setup, "source_field", {})
        for f in setup.fields_in_put_order(setup.input_field, early):
            # (a field received on its model's grid: the coupler fills the source array)
            coupler.get(f.name, current_time, sources.get(f.name, lf.field[f.slot]))
        regridded = [f for f in setup.input_field if f.early == early and _regridded(lf, f)]
        if any(f.name in sources for f in regridded):
            engine.receive(phase)  # do_regridding reads the received fields as last gathered
        for f in regridded:
            engine.do_regridding(f.var, f.surface_type)
        engine.step(phase, current_time)
        if debug:
            _log_ranges(setup, engine, early, current_time, log)
        if budgets is not None:
            _log_budgets(setup, engine, early, phase, current_time, budgets)
        for f in setup.fields_in_put_order(setup.output_field, early):
            coupler.put(f.name, current_time, lf.field[f.slot])


def run(setup, engine, coupler, num_timesteps=None, timestep=None, log=None, budgets=None):
    """DO n_timestep = 1, num_timesteps; current_time = (n_timestep - 1) * timestep.
    log, budgets: see coupling_step."""
    n = setup.nml["num_timesteps"] if num_timesteps is None else num_timesteps
    dt = setup.nml["timestep"] if timestep is None else timestep
    for k in range(1, n + 1):
        coupling_step(setup, engine, coupler, (k - 1) * dt, log=log, budgets=budgets)


__all__ = ["coupling_step", "run"]
