"""Guard-band harness: every array of a case carved out of ONE allocation, sentinel bands
between the arrays, so that a store past an output, a load past an input or a write into an
input shows up (tests/test_guards.py on the CPU, tests/test_gpu_guard_bands.py on the GPU).

  * The band on each side of every array is at least BAND = two layout tiles
    (2 << kLayoutShift = 8192 elements): wider than any block tile, chunk or grid-length
    difference the tests use, so every access a correct or an incorrect tail can make stays
    inside the arena's own allocation; a longer overrun lands in the next array, where the
    parity or the input check sees it.
  * Every band element is a quiet NaN whose payload is its own element index in the arena
    (fp64 0x7FF8000000000000 | index, fp32 0x7FC00000 | (index & 0x3FFFFF)): a band that is
    read and used poisons the result, a band that is overwritten -- or copied from a shifted
    position -- differs from its expected bit pattern (integer comparison).
  * An array starts at a chosen offset modulo 16 bytes and ends exactly at its length: the
    band (or, with tail=k, the k sentinel cells the array is longer than its grid) starts at
    element n with no padding.
  * Aliases (one array object in several slots) stay aliases.

Backends: "numpy" (caller heap), "lib" (fcx.host_alloc.Arena, library memory), "torch"
(cuda:0).  Importing this module needs neither a GPU nor the library.
"""
import itertools

import numpy as np

LAYOUT_SHIFT = 12  # kLayoutShift (fcx_internal.h): the engine's mirrors are cut into tiles of 4096 cells
BAND = 2 << LAYOUT_SHIFT
_SLACK = 4  # elements an array start may move to reach its offset modulo 16 bytes

_BITS = {"float64": (np.uint64, 0x7FF8000000000000, (1 << 51) - 1),
         "float32": (np.uint32, 0x7FC00000, 0x3FFFFF)}


def sentinels(dtype, lo, hi):
    """the expected bit patterns of band elements [lo, hi) of an arena"""
    u, quiet, mask = _BITS[dtype]
    return (np.arange(lo, hi, dtype=np.uint64) & np.uint64(mask) | np.uint64(quiet)).astype(u)


def distinct_arrays(case):
    """[(first key, array, grid cells)] of the distinct arrays of a case, in slot order"""
    seen, out = set(), []
    for key, a in case.lf.field.items():
        if id(a) not in seen:
            seen.add(id(a))
            out.append((key, a, case.lf.grid_size[key[1] - 1]))
    return out


def elements_needed(sizes, tail=0):
    return sum(int(n) + tail + BAND + _SLACK for n in sizes) + BAND + _SLACK


class _Region:
    __slots__ = ("key", "start", "n", "length", "output", "snap", "inner")

    def __init__(self, key, start, n, length, output):
        self.key, self.start, self.n, self.length, self.output = key, start, n, length, output
        self.snap, self.inner = None, []


class GuardedArena:
    """One allocation of `capacity` elements, all sentinels until arrays are carved out of it.

    offset : byte offset of the array starts modulo 16 (fp64: 0 or 8; fp32: 0, 4, 8 or 12)
    only   : None -- every array starts at `offset`; a key -- that array alone does, all
             others at 0
    tail   : every array is bound `tail` elements longer than its grid; the tail holds
             sentinels and must stay bit-unchanged
    """

    def __init__(self, backend, dtype, capacity, offset=0, only=None, tail=0):
        if dtype not in _BITS:
            raise ValueError(f"dtype {dtype}: float64 or float32")
        self.backend, self.dtype, self.capacity = backend, dtype, int(capacity)
        self.es = np.dtype(dtype).itemsize
        if offset % self.es or not 0 <= offset < 16:
            raise ValueError(f"offset {offset}: a multiple of {self.es} below 16")
        self.offset, self.only, self.tail = offset, only, int(tail)
        self.regions = []
        self._cursor = 0
        self._lib = None
        image = sentinels(dtype, 0, self.capacity).view(dtype)
        if backend == "numpy":
            self.buf = image
            self.base = self.buf.ctypes.data
        elif backend == "lib":
            from fcx import host_alloc

            self._lib = host_alloc.Arena()
            self.buf = self._lib.empty(self.capacity, dtype)
            self.buf.view(_BITS[dtype][0])[:] = image.view(_BITS[dtype][0])
            self.base = self.buf.ctypes.data
        elif backend == "torch":
            import torch

            self.buf = torch.from_numpy(image).to("cuda:0")
            self.base = self.buf.data_ptr()
        else:
            raise ValueError(f"backend {backend}")

    # ---- building
    @classmethod
    def for_cases(cls, cases, backend, extra=(), offset=0, only=None, tail=0):
        """An arena sized for the arrays of the cases plus extra arrays of the given sizes,
        with the cases' arrays moved in (interleaved when there are several cases)."""
        cases = list(cases)
        dtype = cases[0].lf.dtype
        sizes = [n for c in cases for _, _, n in distinct_arrays(c)] + [int(n) for n in extra]
        arena = cls(backend, dtype, elements_needed(sizes, tail), offset, only, tail)
        arena.adopt(*cases)
        if only is not None and not any(r.key == only for r in arena.regions):
            raise KeyError(f"only={only}: no array of that key")
        return arena

    @classmethod
    def for_case(cls, case, backend, **kw):
        return cls.for_cases([case], backend, **kw)

    def _carve(self, key, n, tail, output):
        off = self.offset if self.only is None or self.only == key else 0
        start = self._cursor + BAND
        while (self.base + start * self.es) % 16 != off:
            start += 1
        length = int(n) + tail
        if start + length + BAND > self.capacity:
            raise ValueError("GuardedArena: capacity too small for another array and its band")
        self._cursor = start + length
        r = _Region(key, start, int(n), length, bool(output))
        self.regions.append(r)
        return r, self.buf[start:start + length]

    def _store(self, r, values):
        view = self.buf[r.start:r.start + r.n]
        if self.backend == "torch":
            import torch

            host = values if isinstance(values, np.ndarray) else values.detach().cpu().numpy()
            view.copy_(torch.from_numpy(np.ascontiguousarray(host[:r.n], dtype=self.dtype)))
        else:
            view[:] = values[:r.n]

    def adopt(self, *cases):
        """Move every distinct array of the cases into the arena and rebind the views into
        case.lf.field; with several cases the arrays are interleaved and keyed (i, s, g, name)."""
        many = len(cases) > 1
        lists = [distinct_arrays(c) for c in cases]
        moved = [dict() for _ in cases]
        outs = [{id(c.lf.field[k]) for k in c.outputs} for c in cases]
        for row in itertools.zip_longest(*lists):
            for i, item in enumerate(row):
                if item is None:
                    continue
                key, a, n = item
                if str(a.dtype).replace("torch.", "") != self.dtype:
                    raise TypeError(f"{key}: {a.dtype} array in a {self.dtype} arena")
                if a.shape[0] != n:
                    raise ValueError(f"{key}: {a.shape[0]} cells on a grid of {n}")
                r, view = self._carve((i,) + key if many else key, n, self.tail, id(a) in outs[i])
                self._store(r, a)
                moved[i][id(a)] = view
        for i, c in enumerate(cases):
            for key, a in list(c.lf.field.items()):
                c.lf.field[key] = moved[i][id(a)]
        return self

    def empty(self, n, key, output=True, tail=None):
        """Another array of n elements from the arena (atmosphere and remap outputs, the shared
        boundary buffer), NaN-filled; output=False makes it a pure input for snapshot()."""
        r, view = self._carve(key, n, self.tail if tail is None else tail, output)
        self._store(r, np.full(int(n), np.nan, dtype=self.dtype))
        return view

    def protect(self, key, lo, hi):
        """Cells [lo, hi) of array `key` become band: sentinels that must stay bit-unchanged."""
        r = self.region(key)
        if not 0 <= lo <= hi <= r.n:
            raise ValueError(f"{key}: [{lo}, {hi}) outside its {r.n} cells")
        r.inner.append((lo, hi))
        img = sentinels(self.dtype, r.start + lo, r.start + hi).view(self.dtype)
        if self.backend == "torch":
            import torch

            self.buf[r.start + lo:r.start + hi].copy_(torch.from_numpy(img))
        else:
            self.buf.view(_BITS[self.dtype][0])[r.start + lo:r.start + hi] = img.view(_BITS[self.dtype][0])

    def region(self, key):
        for r in self.regions:
            if r.key == key:
                return r
        raise KeyError(key)

    # ---- checking
    def bits(self):
        """the whole arena's bit patterns on the host"""
        u = _BITS[self.dtype][0]
        if self.backend == "torch":
            return self.buf.cpu().numpy().view(u)
        return np.array(self.buf.view(u), copy=True)

    def snapshot(self):
        """Record the bit patterns of every array a run must not write: all but the cases'
        outputs (case.outputs, from the method tables) and the declared extra outputs."""
        bits = self.bits()
        for r in self.regions:
            r.snap = None if r.output else bits[r.start:r.start + r.n].copy()
        return self

    def band_elements(self):
        """elements check() compares against their sentinel pattern"""
        inside = sum(r.n - sum(hi - lo for lo, hi in r.inner) for r in self.regions)
        return self.capacity - inside

    def check(self):
        """[(key, side, first offending offset, count)], empty when the run was clean.
        side "before": offset < 0 counts back from the array's first cell; "after": offset >= 0
        counts from the first element past the array's grid cells (the tail, then the band);
        "inside": a protected range of the array, offset = the cell; "input changed": an array
        no plan may write differs from its snapshot, offset = the first changed cell."""
        bits = self.bits()
        bad = bits != sentinels(self.dtype, 0, self.capacity)
        out = []
        regs = sorted(self.regions, key=lambda r: r.start)
        for i, r in enumerate(regs):
            prev_end = regs[i - 1].start + regs[i - 1].n if i else 0
            nxt = regs[i + 1].start if i + 1 < len(regs) else self.capacity
            end = r.start + r.n
            # the band between two arrays: its half nearer to an array is named after that array
            lo = prev_end + (r.start - prev_end) // 2 if i else 0
            hi = end + (nxt - end) // 2 if i + 1 < len(regs) else self.capacity
            w = np.nonzero(bad[lo:r.start])[0]
            if w.size:
                out.append((r.key, "before", int(lo + w[0] - r.start), int(w.size)))
            w = np.nonzero(bad[end:hi])[0]
            if w.size:
                out.append((r.key, "after", int(w[0]), int(w.size)))
            for a, z in r.inner:
                w = np.nonzero(bad[r.start + a:r.start + z])[0]
                if w.size:
                    out.append((r.key, "inside", int(a + w[0]), int(w.size)))
            if r.snap is not None:
                keep = np.ones(r.n, dtype=bool)
                for a, z in r.inner:
                    keep[a:z] = False
                w = np.nonzero((bits[r.start:end] != r.snap) & keep)[0]
                if w.size:
                    out.append((r.key, "input changed", int(w[0]), int(w.size)))
        return out

    def host(self, view, n=None):
        """a host copy of the first n cells (default: all) of one of the arena's views"""
        a = view.detach().cpu().numpy() if self.backend == "torch" else np.array(view, copy=True)
        return a if n is None else a[:n]

    def outputs(self, case):
        """{key: host copy of the grid cells} of a case's outputs (the tail left out)"""
        return {k: self.host(case.lf.field[k], case.lf.grid_size[k[1] - 1]) for k in case.outputs}

    def close(self):
        self.buf = None
        if self._lib is not None:
            self._lib.close()
            self._lib = None
