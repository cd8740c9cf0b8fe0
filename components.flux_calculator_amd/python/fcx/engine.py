"""Engine: one libfcx engine bound to a LocalFields (one rank, one GPU)."""
import collections
import ctypes
import warnings

import numpy as np

from . import _lib
from .basic import FLUX_ID, IDX, METHOD_ID, PHASE_ALL, PHASE_EARLY, PHASE_NORMAL
from .local_field import LocalFields, data_ptr, dtype_name, is_device


FieldRange = collections.namedtuple("FieldRange", "min max n_nan n_inf first_bad")
FieldRange.__doc__ = """struct fcx_field_range: min / max over the cells that are not NaN (both NaN when
there is none), the NaN and Inf counts, the lowest cell holding either (-1: none)."""


def _ranges(buf, n):
    return [FieldRange(r.min, r.max, r.n_nan, r.n_inf, r.first_bad) for r in buf[:n]]


class ExactSum:
    """struct fcx_exact_sum as a value: an exact sum of doubles (a fixed-point long accumulator of
    68 limbs, value = sum_k limbs[k] * 2**(32 k - 1088)) with the counts of the terms that are in
    it (n_terms) and of those left out (n_nan, n_pinf, n_ninf).  Always canonical, so two sums are
    equal iff bytes(a) == bytes(b).  a + b merges (fcx_sum_merge); .value rounds once
    (fcx_sum_value).  Needs neither a GPU nor an engine."""

    __slots__ = ("c",)

    def __init__(self, c=None):
        self.c = _lib.ExactSumC()
        if c is not None:
            ctypes.memmove(ctypes.byref(self.c), ctypes.byref(c), ctypes.sizeof(_lib.ExactSumC))

    @classmethod
    def of(cls, x, area=None):
        """The host twin of the device kernel: the exact sum of x (float64 or float32), or of
        the IEEE products area[j] * x[j]."""
        return cls().add_terms(x, area)

    def add_terms(self, x, area=None):
        x = np.ascontiguousarray(x)
        if x.dtype not in (np.float64, np.float32) or x.ndim != 1:
            raise TypeError("ExactSum: a 1-D float64 or float32 array")
        a = None
        if area is not None:
            a = np.ascontiguousarray(area, dtype=np.float64)
            if a.shape != x.shape:
                raise ValueError("ExactSum: one area per term")
        fn = _lib.load().fcx_sum_add_terms_f32 if x.dtype == np.float32 else _lib.load().fcx_sum_add_terms
        _lib.check(fn(self.c, ctypes.c_void_p(x.ctypes.data), ctypes.c_void_p(a.ctypes.data) if a is not None else None,
                      x.shape[0]))
        return self

    @classmethod
    def from_raw(cls, words):
        """72 int64 words (68 limbs, 4 counts), e.g. the MPI_SUM of the ranks' canonical sums,
        normalised once."""
        w = np.ascontiguousarray(words, dtype=np.int64).reshape(-1)
        if w.shape[0] != _lib.FCX_SUM_LIMBS + 4:
            raise ValueError("ExactSum.from_raw: 72 int64 words")
        raw = _lib.ExactSumC.from_buffer_copy(w.tobytes())
        out = cls()
        _lib.check(_lib.load().fcx_sum_merge(out.c, raw))
        return out

    def words(self):
        """the 72 int64 words of the struct (what a host adds across ranks)"""
        return np.frombuffer(bytes(self), dtype=np.int64).copy()

    @property
    def value(self):
        v = ctypes.c_double()
        _lib.check(_lib.load().fcx_sum_value(self.c, ctypes.byref(v)))
        return v.value

    @property
    def limbs(self):
        return list(self.c.limb)

    n_terms = property(lambda self: self.c.n_terms)
    n_nan = property(lambda self: self.c.n_nan)
    n_pinf = property(lambda self: self.c.n_pinf)
    n_ninf = property(lambda self: self.c.n_ninf)

    def __neg__(self):
        """the sum of the negated terms (an infinity's count changes sides)"""
        w = self.words()
        w[:_lib.FCX_SUM_LIMBS] = -w[:_lib.FCX_SUM_LIMBS]
        w[-2], w[-1] = w[-1], w[-2]
        return ExactSum.from_raw(w)

    def __add__(self, other):
        if not isinstance(other, ExactSum):
            return NotImplemented
        out = ExactSum(self.c)
        _lib.check(_lib.load().fcx_sum_merge(out.c, other.c))
        return out

    def __bytes__(self):
        return ctypes.string_at(ctypes.byref(self.c), ctypes.sizeof(_lib.ExactSumC))

    def __eq__(self, other):
        return isinstance(other, ExactSum) and bytes(self) == bytes(other)

    def __hash__(self):
        return hash(bytes(self))

    def __repr__(self):
        return (f"ExactSum(value={self.value!r}, n_terms={self.n_terms}, n_nan={self.n_nan}, "
                f"n_pinf={self.n_pinf}, n_ninf={self.n_ninf})")


class Engine:
    """Binds every slot of a LocalFields to a new libfcx engine and commits it.

    methods: {which_table_name: [method string per surface type 1..T]}
    corrections: None or (init_date, array) with array shaped like the Fortran
        corrections(1, 12, grid_size(1)) -> numpy [n][12] (cell-major) or [12][n].
    averages: iterable of (phase, grid, name) type-0 outputs averaged before their put.
    """

    def __init__(self, lf: LocalFields, num_surface_types, methods, corrections=None,
                 averages=(), regrid=None, device=0, stream=None, atmos=None, options=None, remaps=None,
                 lib=None, commit=True, use_constants=True, output_use=None, received=None):
        """atmos: exchange -> atmosphere accumulation, dict with
             local   : fcx.parallel.LocalAtmos of this rank
             fields  : [(phase, surface_type, grid, name, out_array[n_atmos])]
             shared  : optional (device_buffer[n_boundaries * stride], stride)
             own_boundaries : optional True: the engine allocates its boundary slots
                       (fcx_set_atmos_boundaries) from local.n_boundaries/left/right
             comm    : optional fcx.comm.Comm: the engine completes its boundary slots
                       itself after every accumulation (fcx_set_comm)
             invariant : optional True: FCX_OPT_ATMOS_INVARIANT with local.max_terms and
                       local.left_pos (fcx_set_atmos_terms): shared atmosphere cells have the
                       bits of a one-rank engine; a `shared` buffer then needs a stride of
                       fields x (1 + max_terms) doubles (Engine.atmos_columns)
        remaps: exchange -> model remaps, each {"n_dst", "src", "dst", "w" (0-based links),
                 "fields": [(phase, surface_type, grid, name, out_array[n_dst])]}
        options: {name: value} for fcx_set_option.
        lib: another libfcx build from _lib.load_path (A/B measurement tools only).
        commit=False: bind only (no GPU touched); plan_check() then audits the plans on the host.
        use_constants: the fields lf.constant records (namelist val_* values) are declared with
             fcx_bind_constant after their arrays are bound, so the engine never transfers them;
             a recorded field whose array no longer holds the value in every cell (a host that
             wrote it after set-up) stays an ordinary array, with a RuntimeWarning and an entry
             in Engine.dropped_constants.  False: every field is an array.
        output_use: {(surface_type, grid, name): use} declared with fcx_set_output_use after the
             arrays are bound; use is _lib.FCX_OUT_HOST / FCX_OUT_DEVICE / FCX_OUT_UNREAD or one
             of "host", "device", "unread".  The arrays of the declared slots are neither written
             nor read by the engine from the commit on.
        received: model grid -> exchange grid maps of received fields, each {"grid", "n_src",
             "src", "dst", "w" (0-based links), "fields": [(phase, surface_type, grid, name,
             src_array[n_src])]}: the host receives the field on the model's grid into src_array
             and the engine gathers it to the exchange grid on the device (fcx_bind_received).
             The exchange-grid arrays of the declared slots, and of every slot aliasing them, are
             neither read nor written by the engine from the commit on."""
        self.lib = lib if lib is not None else _lib.load()
        self.lf = lf
        self.T = int(num_surface_types)
        self.methods = {k: list(v) for k, v in methods.items()}
        self._keep = []
        # the accumulated fields, (phase, surface_type, grid, name) in registration order (the
        # order of atmos_integrals), and whether their cells' areas were set
        self.atmos_fields = [(int(p), int(s), int(g), name) for p, s, g, name, _ in (atmos or {}).get("fields", ())]
        self.atmos_areas_set = False
        h = ctypes.c_void_p()
        gs = (ctypes.c_int32 * 3)(*lf.grid_size)
        _lib.check(self.lib.fcx_create(device, self.T, gs, ctypes.byref(h)))
        self.h = h
        try:
            if stream is not None:
                _lib.check(self.lib.fcx_set_stream(h, ctypes.c_void_p(stream)))
            dtype = getattr(lf, "dtype", "float64")
            self.precision = dtype
            _lib.check(self.lib.fcx_set_precision(
                h, _lib.FCX_PRECISION_F32 if dtype == "float32" else _lib.FCX_PRECISION_F64))
            for table, per_type in self.methods.items():
                for s, m in enumerate(per_type[: self.T], start=1):
                    mid = METHOD_ID[m.rstrip()] if isinstance(m, str) else int(m)
                    _lib.check(self.lib.fcx_set_method(h, FLUX_ID[table], s, mid))
            for s, g, var, a, alloc in lf.slots():
                flags = (_lib.FCX_MEM_DEVICE if is_device(a) else _lib.FCX_MEM_HOST)
                if alloc:
                    flags |= _lib.FCX_ALLOCATED
                if dtype_name(a) != dtype:
                    raise TypeError(f"slot {(s, g, var)}: {dtype_name(a)} array in a {dtype} LocalFields")
                n = a.shape[0]
                _lib.check(self.lib.fcx_bind_field(h, s, g, var, ctypes.c_void_p(data_ptr(a)), n, flags))
            self.constants = {}  # (s, g, name) -> value of the slots declared constant
            self.dropped_constants = {}  # recorded constants whose array no longer holds the value
            if use_constants:
                for (s, g, name), value in getattr(lf, "constant", {}).items():
                    a = lf.field.get((s, g, name))
                    if a is None or not bool((a == value).all()):
                        # the Fortran drop-in stops here (fcx_declare_constant); a Python host may
                        # have rewritten the field on purpose, so it is told and the array is used
                        self.dropped_constants[(s, g, name)] = float(value)
                        warnings.warn(f"{name}({s},{g}) is recorded as the constant {value} but its array "
                                      "no longer holds it in every cell: bound as an ordinary array",
                                      RuntimeWarning, stacklevel=2)
                        continue
                    _lib.check(self.lib.fcx_bind_constant(h, s, g, IDX[name], float(value)))
                    self.constants[(s, g, name)] = float(value)
            self.output_use = {}  # (s, g, name) -> use of the slots declared with fcx_set_output_use
            for (s, g, name), use in (output_use or {}).items():
                self.set_output_use(s, g, name, use)
            if corrections is not None:
                init_date, corr = corrections
                corr = np.ascontiguousarray(corr, dtype=np.float64)
                layout = _lib.FCX_CORR_CELL_MAJOR if corr.shape[-1] == 12 else _lib.FCX_CORR_MONTH_MAJOR
                self._keep.append(corr)
                _lib.check(self.lib.fcx_set_corrections(h, 1, int(init_date), ctypes.c_void_p(corr.ctypes.data),
                                                        lf.grid_size[0], layout))
            if regrid:
                for which, (src, dst, w) in regrid.get("matrices", {}).items():
                    src = np.ascontiguousarray(src, dtype=np.int32)
                    dst = np.ascontiguousarray(dst, dtype=np.int32)
                    w = np.ascontiguousarray(w, dtype=np.float64)
                    self._keep += [src, dst, w]
                    _lib.check(self.lib.fcx_set_regrid_matrix(
                        h, which, src.shape[0], ctypes.c_void_p(src.ctypes.data),
                        ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(w.ctypes.data)))
            for (s, g, name), mask in lf.put_to.items():
                _lib.check(self.lib.fcx_set_put_to(h, s, g, IDX[name], mask))
            for phase, g, name in averages:
                _lib.check(self.lib.fcx_add_average(h, phase, g, IDX[name]))
            if atmos is not None:
                la = atmos["local"]
                idx = np.ascontiguousarray(la.atmos_index, dtype=np.int32)
                w = np.ascontiguousarray(la.weight, dtype=np.float64)
                self._keep += [idx, w]
                _lib.check(self.lib.fcx_set_atmos_map(h, la.n_atmos, ctypes.c_void_p(idx.ctypes.data),
                                                      ctypes.c_void_p(w.ctypes.data)))
                for phase, s, g, name, out in atmos["fields"]:
                    if dtype_name(out) != dtype:
                        raise TypeError(f"atmosphere output {name}: {dtype_name(out)} array in a {dtype} engine")
                    flags = _lib.FCX_MEM_DEVICE if is_device(out) else _lib.FCX_MEM_HOST
                    self._keep.append(out)
                    _lib.check(self.lib.fcx_add_atmos_field(h, phase, s, g, IDX[name],
                                                            ctypes.c_void_p(data_ptr(out)), flags))
                if atmos.get("invariant"):
                    # sums that do not depend on the number of ranks: the boundary slots carry
                    # the shared cells' terms (max_terms term columns per field)
                    _lib.check(self.lib.fcx_set_option(h, _lib.FCX_OPT_ATMOS_INVARIANT, 1))
                    _lib.check(self.lib.fcx_set_atmos_terms(h, int(la.max_terms), int(la.left_pos)))
                if atmos.get("shared") is not None:
                    buf, stride = atmos["shared"]
                    self._keep.append(buf)
                    _lib.check(self.lib.fcx_set_atmos_shared(h, ctypes.c_void_p(data_ptr(buf)), la.n_boundaries,
                                                             stride, la.left, la.right))
                elif atmos.get("own_boundaries"):
                    _lib.check(self.lib.fcx_set_atmos_boundaries(h, la.n_boundaries, la.left, la.right))
                if atmos.get("comm") is not None:
                    self._keep.append(atmos["comm"])
                    _lib.check(self.lib.fcx_set_comm(h, atmos["comm"].h))
            for rm in remaps or ():
                src = np.ascontiguousarray(rm["src"], dtype=np.int32)
                dst = np.ascontiguousarray(rm["dst"], dtype=np.int32)
                w = np.ascontiguousarray(rm["w"], dtype=np.float64)
                self._keep += [src, dst, w]
                rid = ctypes.c_int32()
                _lib.check(self.lib.fcx_add_remap(h, int(rm["n_dst"]), src.shape[0], ctypes.c_void_p(src.ctypes.data),
                                                  ctypes.c_void_p(dst.ctypes.data), ctypes.c_void_p(w.ctypes.data),
                                                  ctypes.byref(rid)))
                for phase, s, g, name, out in rm["fields"]:
                    if dtype_name(out) != dtype:
                        raise TypeError(f"remap output {name}: {dtype_name(out)} array in a {dtype} engine")
                    flags = _lib.FCX_MEM_DEVICE if is_device(out) else _lib.FCX_MEM_HOST
                    self._keep.append(out)
                    _lib.check(self.lib.fcx_add_remap_field(h, rid.value, phase, s, g, IDX[name],
                                                            ctypes.c_void_p(data_ptr(out)), flags))
            self.receive_maps = []  # map id of every entry of `received`
            for rm in received or ():
                mid = self.add_receive_map(rm["grid"], rm["n_src"], rm["src"], rm["dst"], rm["w"])
                for phase, s, g, name, src_array in rm.get("fields", ()):
                    self.bind_received(mid, phase, s, g, name, src_array)
            for name, value in (options or {}).items():
                _lib.check(self.lib.fcx_set_option(h, self._option_id(name), int(value)))
            if commit:
                _lib.check(self.lib.fcx_commit(h))
        except Exception:
            self.lib.fcx_destroy(h)
            self.h = None
            raise

    def plan_check(self):
        """fcx_plan_check: every launch plan built on the host and audited (before commit)."""
        _lib.check(self.lib.fcx_plan_check(self.h))

    def commit(self):
        _lib.check(self.lib.fcx_commit(self.h))

    # ---- fused path
    def upload(self, phase=PHASE_ALL):
        _lib.check(self.lib.fcx_upload(self.h, phase))

    def run(self, phase=PHASE_ALL, current_step_time=0):
        _lib.check(self.lib.fcx_run(self.h, phase, int(current_step_time)), self.h, self.lib)

    def download(self, phase=PHASE_ALL):
        _lib.check(self.lib.fcx_download(self.h, phase))

    def step(self, phase=PHASE_ALL, current_step_time=0):
        _lib.check(self.lib.fcx_step(self.h, phase, int(current_step_time)), self.h, self.lib)

    def step_async(self, phase=PHASE_ALL, current_step_time=0):
        """fcx_step_async: the step queued; the host arrays hold the outputs after synchronize()."""
        _lib.check(self.lib.fcx_step_async(self.h, phase, int(current_step_time)), self.h, self.lib)

    def upload_field(self, surface_type, grid, name):
        """fcx_upload_field: one input field handed over (staged by the engine's upload thread)."""
        _lib.check(self.lib.fcx_upload_field(self.h, int(surface_type), int(grid), IDX[name]))

    def set_stream(self, stream):
        """fcx_set_stream: launch on this HIP stream (a raw hipStream_t, e.g. a torch
        stream's .cuda_stream) from now on, e.g. a capturing stream for a HIP graph."""
        _lib.check(self.lib.fcx_set_stream(self.h, ctypes.c_void_p(stream)))

    def do_regridding(self, name, surface_type=0):
        """do_regridding (basic:463-522) of one variable, host arrays in and out."""
        _lib.check(self.lib.fcx_do_regridding(self.h, IDX[name], int(surface_type)))

    def synchronize(self):
        _lib.check(self.lib.fcx_synchronize(self.h), self.h, self.lib)

    def last_kernel_ms(self):
        ms = ctypes.c_float()
        _lib.check(self.lib.fcx_last_kernel_ms(self.h, ctypes.byref(ms)))
        return ms.value

    def algorithmic_bytes(self, phase=PHASE_ALL):
        b = ctypes.c_int64()
        _lib.check(self.lib.fcx_algorithmic_bytes(self.h, phase, ctypes.byref(b)))
        return b.value

    def staging_bytes(self):
        """bytes of the page-locked staging arena of caller heap arrays (fcx_staging_bytes)"""
        b = ctypes.c_int64()
        _lib.check(self.lib.fcx_staging_bytes(self.h, ctypes.byref(b)))
        return b.value

    def zero_copy_bytes(self):
        """bytes of host arrays the kernels use in place (fcx_zero_copy_bytes)"""
        b = ctypes.c_int64()
        _lib.check(self.lib.fcx_zero_copy_bytes(self.h, ctypes.byref(b)))
        return b.value

    def span_runs(self, phase=PHASE_ALL):
        """(uploads, downloads) one step of the phase makes of the fcx_host_malloc arrays with
        the span transport (fcx_span_runs)"""
        a, b = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.fcx_span_runs(self.h, phase, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value

    def zero_copy_active(self):
        return self.zero_copy_bytes() > 0

    OPTIONS = {"cells_per_thread": 1, "max_blocks": 2, "nontemporal": 3, "specialize": 4,
               "atmos_in_run": 5, "pipeline_chunks": 7, "pipeline_min_chunk": 8, "zero_copy": 9,
               "timing": 10, "tiled_layout": 11, "remap_pack": 13, "host_staging": 15, "host_threads": 16,
               "atmos_halo": 17, "deferred_scatter": 18, "lib_spans": 19, "atm_records": 21,
               "f32_math": _lib.FCX_OPT_F32_MATH, "check_finite": _lib.FCX_OPT_CHECK_FINITE,
               "cr_math": _lib.FCX_OPT_CR_MATH, "sum_baseline": _lib.FCX_OPT_SUM_BASELINE,
               "atmos_invariant": _lib.FCX_OPT_ATMOS_INVARIANT}

    def run_atmos(self, phase=PHASE_ALL):
        _lib.check(self.lib.fcx_run_atmos(self.h, phase))

    def atmos_finish(self):
        """After the all-reduce of the shared boundary buffer (fcx_atmos_finish)."""
        _lib.check(self.lib.fcx_atmos_finish(self.h))

    def remap_info(self, remap_id=0):
        """(scatter, packed) of a remap (fcx_remap_info): packed 0 = gather from the arrays,
        1 = packing pass, 2 = records written by the last run's flux launch."""
        sc, pk = ctypes.c_double(), ctypes.c_int32()
        _lib.check(self.lib.fcx_remap_info(self.h, remap_id, ctypes.byref(sc), ctypes.byref(pk)))
        return sc.value, pk.value

    @classmethod
    def _option_id(cls, name):
        """an OPTIONS name, or a raw enum fcx_option value (measurement builds' extra knobs)"""
        if isinstance(name, int) or (isinstance(name, str) and name.isdigit()):
            return int(name)
        return cls.OPTIONS[name]

    def set_option(self, name, value):
        _lib.check(self.lib.fcx_set_option(self.h, self._option_id(name), int(value)))

    def device_ptr(self, s, g, name):
        p = ctypes.POINTER(ctypes.c_double)()
        _lib.check(self.lib.fcx_device_ptr(self.h, s, g, IDX[name], ctypes.byref(p)))
        return ctypes.cast(p, ctypes.c_void_p).value

    def constant_info(self, s, g, name):
        """fcx_constant_info: 0 the slot is an array, 1 a constant without a device array, 2 a
        constant in a device array the engine filled at commit."""
        k = ctypes.c_int32()
        _lib.check(self.lib.fcx_constant_info(self.h, int(s), int(g), IDX[name], ctypes.byref(k)))
        return k.value

    def bind_constant(self, s, g, name, value):
        """fcx_bind_constant on an uncommitted engine (commit=False)."""
        _lib.check(self.lib.fcx_bind_constant(self.h, int(s), int(g), IDX[name], float(value)))
        self.constants[(s, g, name)] = float(value)

    def add_receive_map(self, grid, n_src, src, dst, w):
        """fcx_add_receive_map on an uncommitted engine: 0-based links model cell -> exchange cell
        of `grid`; returns the map id."""
        src = np.ascontiguousarray(src, dtype=np.int32)
        dst = np.ascontiguousarray(dst, dtype=np.int32)
        w = np.ascontiguousarray(w, dtype=np.float64)
        if not (src.shape == dst.shape == w.shape and src.ndim == 1):
            raise ValueError("receive map: src, dst and w must be 1-D arrays of one length")
        mid = ctypes.c_int32()
        _lib.check(self.lib.fcx_add_receive_map(self.h, int(grid), int(n_src), src.shape[0],
                                                ctypes.c_void_p(src.ctypes.data), ctypes.c_void_p(dst.ctypes.data),
                                                ctypes.c_void_p(w.ctypes.data), ctypes.byref(mid)))
        self.receive_maps.append(mid.value)
        return mid.value

    def bind_received(self, map_id, phase, s, g, name, src_array):
        """fcx_bind_received on an uncommitted engine: slot (s, g, name) is received into
        src_array (model grid) before `phase` and gathered through map `map_id`."""
        if dtype_name(src_array) != self.precision:
            raise TypeError(f"received source of {name}: {dtype_name(src_array)} array in a {self.precision} engine")
        flags = _lib.FCX_MEM_DEVICE if is_device(src_array) else _lib.FCX_MEM_HOST
        self._keep.append(src_array)
        _lib.check(self.lib.fcx_bind_received(self.h, int(map_id), int(phase), int(s), int(g), IDX[name],
                                              ctypes.c_void_p(data_ptr(src_array)), src_array.shape[0], flags))

    def receive(self, phase=PHASE_ALL):
        """fcx_receive: the phase's sources uploaded and gathered, nothing else (hosts that go on
        with the per-call subroutines)."""
        _lib.check(self.lib.fcx_receive(self.h, int(phase)))

    def received_info(self, s, g, name):
        """fcx_received_info: (kind, map id): kind 0 the slot is not received (map id -1), 1 it is
        gathered into a device array of the engine's by a gather launch."""
        k, m = ctypes.c_int32(), ctypes.c_int32()
        _lib.check(self.lib.fcx_received_info(self.h, int(s), int(g), IDX[name], ctypes.byref(k), ctypes.byref(m)))
        return k.value, m.value

    OUTPUT_USE = {"host": _lib.FCX_OUT_HOST, "device": _lib.FCX_OUT_DEVICE, "unread": _lib.FCX_OUT_UNREAD}

    def set_output_use(self, s, g, name, use):
        """fcx_set_output_use on an uncommitted engine: what the host does with a computed output."""
        use = self.OUTPUT_USE[use] if isinstance(use, str) else int(use)
        _lib.check(self.lib.fcx_set_output_use(self.h, int(s), int(g), IDX[name], use))
        self.output_use[(s, g, name)] = use

    def output_info(self, s, g, name):
        """fcx_output_info: 0 the host reads the output, 1 it is kept in a device array, 2 the
        last whole-phase plan built for it left its store out."""
        k = ctypes.c_int32()
        _lib.check(self.lib.fcx_output_info(self.h, int(s), int(g), IDX[name], ctypes.byref(k)))
        return k.value

    def device_layout(self):
        """(tile, tile_stride) of the engine-owned mirrors: cell j of a device buffer is at
        element (j // tile) * tile_stride + j % tile (fcx_device_layout)."""
        tile, stride = ctypes.c_int64(), ctypes.c_int64()
        _lib.check(self.lib.fcx_device_layout(self.h, ctypes.byref(tile), ctypes.byref(stride)))
        return tile.value, stride.value

    def last_group_size(self):
        """Engines in the merged launch of this engine's last fcx_run_group (0: ran as fcx_run)."""
        m = ctypes.c_int32()
        _lib.check(self.lib.fcx_last_group_size(self.h, ctypes.byref(m)))
        return m.value

    def atm_records(self):
        """True when the atmosphere outputs are kept as per-cell records (fcx_atm_records)."""
        on = ctypes.c_int32()
        _lib.check(self.lib.fcx_atm_records(self.h, ctypes.byref(on)))
        return bool(on.value)

    def f32_math(self):
        """True when this is an fp32 engine computing its fluxes in double (fcx_f32_math)."""
        on = ctypes.c_int32()
        _lib.check(self.lib.fcx_f32_math(self.h, ctypes.byref(on)))
        return bool(on.value)

    def cr_math(self):
        """True when this is a committed fp64 engine whose exp and Exner power are correctly
        rounded (fcx_cr_math)."""
        on = ctypes.c_int32()
        _lib.check(self.lib.fcx_cr_math(self.h, ctypes.byref(on)))
        return bool(on.value)

    def atmos_invariant(self):
        """True when FCX_OPT_ATMOS_INVARIANT is on (fcx_atmos_invariant)."""
        on = ctypes.c_int32()
        _lib.check(self.lib.fcx_atmos_invariant(self.h, ctypes.byref(on)))
        return bool(on.value)

    def last_terms_group(self):
        """Engines whose terms shared one launch with this engine's after its last accumulation
        (fcx_last_terms_group; 0: no terms launch)."""
        m = ctypes.c_int32()
        _lib.check(self.lib.fcx_last_terms_group(self.h, ctypes.byref(m)))
        return m.value

    def atmos_columns(self):
        """Doubles per boundary slot (fcx_atmos_columns): the accumulated fields, times
        1 + max_terms with FCX_OPT_ATMOS_INVARIANT."""
        n = ctypes.c_int32()
        _lib.check(self.lib.fcx_atmos_columns(self.h, ctypes.byref(n)))
        return n.value

    def fused_accumulation(self, phase=PHASE_ALL):
        """True when the phase's exchange -> atmosphere accumulation rides inside the flux launch,
        False when atmos_kernel runs it as a second pass (fcx_fused_accumulation)."""
        on = ctypes.c_int32()
        _lib.check(self.lib.fcx_fused_accumulation(self.h, int(phase), ctypes.byref(on)))
        return bool(on.value)

    # ---- field ranges and the non-finite guard
    def field_ranges(self, slots):
        """fcx_field_ranges: a FieldRange per (surface_type, grid, name) of `slots`, in request
        order, of the device buffer behind each slot (the reference's DEBUG MINVAL / MAXVAL lines,
        flux_calculator.F90:879-881, 949-951).  Waits for the engine's stream."""
        slots = list(slots)
        ids = np.array([(int(s), int(g), IDX[name] if isinstance(name, str) else int(name)) for s, g, name in slots],
                       dtype=np.int32).reshape(-1)
        out = (_lib.FieldRangeC * max(len(slots), 1))()
        _lib.check(self.lib.fcx_field_ranges(self.h, len(slots), ctypes.c_void_p(ids.ctypes.data), out))
        return _ranges(out, len(slots))

    def atmos_ranges(self, phase=PHASE_ALL):
        """fcx_atmos_ranges: a FieldRange per atmosphere output of the phase, in registration
        order, read from the device arrays or records as they are."""
        cap = 64
        while True:
            out = (_lib.FieldRangeC * cap)()
            n = ctypes.c_int32()
            rc = self.lib.fcx_atmos_ranges(self.h, int(phase), cap, out, ctypes.byref(n))
            if rc == 1 and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc)
            return _ranges(out, n.value)

    def check_fields(self, phase=PHASE_ALL):
        """fcx_check_fields: the (surface_type, grid, name) slots the non-finite guard checks after
        a run of the phase, inputs first (host only; after plan_check() or commit)."""
        cap = 3 * 11 * 35
        ids = np.zeros(3 * cap, dtype=np.int32)
        n = ctypes.c_int32()
        _lib.check(self.lib.fcx_check_fields(self.h, int(phase), cap, ctypes.c_void_p(ids.ctypes.data), ctypes.byref(n)))
        names = {v: k for k, v in IDX.items()}
        return [(int(ids[3 * k]), int(ids[3 * k + 1]), names[int(ids[3 * k + 2])]) for k in range(n.value)]

    def check_result(self):
        """fcx_check_result of the last checked run: None when it was clean, else a dict."""
        a, s, g, v = ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32(), ctypes.c_int32()
        cell, value = ctypes.c_int64(), ctypes.c_double()
        _lib.check(self.lib.fcx_check_result(self.h, ctypes.byref(a), ctypes.byref(s), ctypes.byref(g), ctypes.byref(v),
                                             ctypes.byref(cell), ctypes.byref(value)))
        if cell.value < 0:
            return None
        names = {i: k for k, i in IDX.items()}
        return {"is_atmos": bool(a.value), "surface_type": s.value, "grid": g.value, "var": v.value,
                "name": names.get(v.value), "cell": cell.value, "value": value.value}

    # ---- exact integrals (flux budgets)
    def set_areas(self, grid, area):
        """fcx_set_areas: the cell areas of exchange grid `grid` (1..3), at least grid_size values;
        before or after commit, and again to replace them."""
        a = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
        _lib.check(self.lib.fcx_set_areas(self.h, int(grid), ctypes.c_void_p(a.ctypes.data), a.shape[0]))

    def set_atmos_areas(self, area):
        """fcx_set_atmos_areas: the areas of the local atmosphere cells; 0.0 for a shared cell
        this rank does not own (fcx.parallel.owned_atmos_mask)."""
        a = np.ascontiguousarray(area, dtype=np.float64).reshape(-1)
        _lib.check(self.lib.fcx_set_atmos_areas(self.h, ctypes.c_void_p(a.ctypes.data), a.shape[0]))
        self.atmos_areas_set = True

    def atmos_twins(self, phase=PHASE_ALL):
        """The (surface_type, grid, name) slots whose accumulation onto the atmosphere grid
        atmos_integrals(phase) integrates, in its order; none while no atmosphere areas are set."""
        if not self.atmos_areas_set:
            return []
        return [(s, g, name) for p, s, g, name in self.atmos_fields if p & int(phase)]

    def field_integrals(self, slots, weighted=True):
        """fcx_field_integrals: an ExactSum per (surface_type, grid, name) of `slots`, in request
        order: the exact sum of the device buffer behind each slot, its terms multiplied by the
        grid's areas when weighted.  Waits for the engine's stream."""
        slots = list(slots)
        ids = np.array([(int(s), int(g), IDX[name] if isinstance(name, str) else int(name)) for s, g, name in slots],
                       dtype=np.int32).reshape(-1)
        out = (_lib.ExactSumC * max(len(slots), 1))()
        _lib.check(self.lib.fcx_field_integrals(self.h, len(slots), ctypes.c_void_p(ids.ctypes.data),
                                                1 if weighted else 0, out))
        return [ExactSum(c) for c in out[:len(slots)]]

    def atmos_integrals(self, phase=PHASE_ALL, weighted=True):
        """fcx_atmos_integrals: an ExactSum per atmosphere output of the phase, in registration
        order, read from the device arrays or records as they are."""
        cap = 64
        while True:
            out = (_lib.ExactSumC * cap)()
            n = ctypes.c_int32()
            rc = self.lib.fcx_atmos_integrals(self.h, int(phase), 1 if weighted else 0, cap, out, ctypes.byref(n))
            if rc == 1 and n.value > cap:
                cap = n.value
                continue
            _lib.check(rc)
            return [ExactSum(c) for c in out[:n.value]]

    def close(self):
        if self.h is not None:
            self.lib.fcx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def run_group(engines, phase=PHASE_ALL, current_step_time=0):
    """fcx_run of every engine, the fused flux passes of the same shape (one surface type, or
    several with the type-0 averages in registers, in any precision) as ONE launch
    (fcx_run_group): the same results as Engine.run of each."""
    if not engines:
        return
    lib = engines[0].lib
    arr = (ctypes.c_void_p * len(engines))(*[e.h.value for e in engines])
    rc = lib.fcx_run_group(arr, len(engines), phase, int(current_step_time))
    if rc == _lib.FCX_E_NONFINITE:  # the first engine in list order whose check found something
        cell = ctypes.c_int64(-1)
        for e in engines:
            lib.fcx_check_result(e.h, None, None, None, None, ctypes.byref(cell), None)
            if cell.value >= 0:
                _lib.check(rc, e.h, lib)
    _lib.check(rc)


def current_month(init_date, seconds):
    """datetime_helpers.get_current_date(...)['current_month'] via libfcx."""
    lib = _lib.load()
    m = ctypes.c_int32()
    _lib.check(lib.fcx_current_month(int(init_date), int(seconds), ctypes.byref(m)))
    return m.value


__all__ = ["Engine", "ExactSum", "FieldRange", "run_group", "current_month", "PHASE_EARLY", "PHASE_NORMAL", "PHASE_ALL"]
