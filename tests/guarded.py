"""Guard-band buffers for contract tests: a matrix or vector inside ONE allocation, with memory the test owns in front of it, behind
it and in the pad columns of every row (row stride ld >= cols).

  Guarded.input(data, ld)          guards and pad columns hold NaN of the element type, the interior holds `data`: a kernel that masks a
                                   ragged edge by multiplying with zero, or reads past an extent, turns its output into NaN
  Guarded.output(rows, cols, ld, dtype[, old])
                                   everything holds a fixed sentinel bit pattern (a NaN with a recognisable payload); with `old` (beta != 0)
                                   the interior holds the old C.  After the call check() asserts, bit-exactly through an integer view, that
                                   the front guard, the back guard and every pad column still hold the sentinel, and names the first
                                   offending (row, col).

The front guard is 64 KiB, the back guard max(64 KiB, 256 rows x ld elements): a store of up to one whole tile too far stays inside
the allocation.  The matrix start is 16-byte aligned.  Vectors ([n] bias, statistics, ...) are matrices of one row.  A plain module
(like stoch_cases.py): works on CPU tensors too, which is how tests/test_guarded_cpu.py checks it."""
from __future__ import annotations

import torch

FRONT_BYTES = 64 * 1024
BACK_BYTES_MIN = 64 * 1024
BACK_ROWS = 256

# sentinel bit patterns: quiet NaNs with a payload no arithmetic produces
_SENTINEL = {1: 0xA5, 2: 0x7FD5, 4: 0x7FD5A5A5}
_INT_VIEW = {1: torch.uint8, 2: torch.int16, 4: torch.int32}


def _signed(pattern: int, size: int) -> int:
    bits = 8 * size
    return pattern - (1 << bits) if size > 1 and pattern >= (1 << (bits - 1)) else pattern


class Guarded:
    """One allocation: [front guard | rows x ld elements | back guard].  `.t` is the [rows, cols] interior view (stride (ld, 1))."""

    def __init__(self, rows: int, cols: int, ld: int, dtype: torch.dtype, device, kind: str):
        assert rows >= 1 and cols >= 1 and ld >= cols, (rows, cols, ld)
        self.rows, self.cols, self.ld, self.dtype, self.kind = rows, cols, ld, dtype, kind
        self.esize = torch.empty((), dtype=dtype).element_size()
        assert FRONT_BYTES % self.esize == 0
        self.front = FRONT_BYTES // self.esize
        self.back = max(BACK_BYTES_MIN // self.esize, BACK_ROWS * ld)
        self.body = rows * ld
        self.raw = torch.empty(self.front + self.body + self.back, dtype=dtype, device=device)
        self.bits = self.raw.view(_INT_VIEW[self.esize])
        # torch allocations are at least 64-byte aligned on every backend used here; the front guard is a multiple of 16 bytes
        assert self.raw.data_ptr() % 16 == 0
        self.t = self.raw[self.front:self.front + self.body].view(rows, ld)[:, :cols]
        self.sentinel = _signed(_SENTINEL[self.esize], self.esize)

    # ---- constructors
    @classmethod
    def input(cls, data: torch.Tensor, ld: int | None = None) -> "Guarded":
        """NaN guards and pad columns around `data` ([rows, cols] or [n])."""
        d2 = data.reshape(1, -1) if data.dim() == 1 else data
        assert d2.dim() == 2 and d2.dtype.is_floating_point
        g = cls(d2.shape[0], d2.shape[1], ld or d2.shape[1], d2.dtype, d2.device, "input")
        g.raw.fill_(float("nan"))
        g.t.copy_(d2)
        return g

    @classmethod
    def output(cls, rows: int, cols: int, ld: int | None, dtype: torch.dtype, device, old: torch.Tensor | None = None) -> "Guarded":
        """sentinel everywhere; the interior holds `old` when given (an accumulating call, beta != 0)"""
        g = cls(rows, cols, ld or cols, dtype, device, "output")
        g.bits.fill_(g.sentinel)
        if old is not None:
            g.t.copy_(old.reshape(rows, cols))
        return g

    @classmethod
    def output_vec(cls, n: int, dtype: torch.dtype, device, old: torch.Tensor | None = None) -> "Guarded":
        return cls.output(1, n, n, dtype, device, old)

    @classmethod
    def output_bytes(cls, nbytes: int, device) -> "Guarded":
        """a workspace of exactly `nbytes` bytes (at least one, so that there is a pointer) between sentinel guards"""
        return cls.output(1, max(int(nbytes), 1), None, torch.uint8, device)

    # ---- access
    def ptr(self) -> int:
        return self.t.data_ptr()

    def vec(self) -> torch.Tensor:
        assert self.rows == 1
        return self.t[0]

    def interior_bits(self) -> torch.Tensor:
        return self.bits[self.front:self.front + self.body].view(self.rows, self.ld)[:, :self.cols]

    # ---- the check
    def violation(self):
        """None, or (region, row, col) of the first element outside the interior that no longer holds the sentinel.  region is "front",
        "pad" or "back"; for "pad" (row, col) is the matrix position (col >= cols), for the guards row is None and col the element
        offset inside the guard."""
        assert self.kind == "output", "only outputs carry a sentinel"
        bad = self.bits[:self.front] != self.sentinel
        if bool(bad.any()):
            return ("front", None, int(torch.nonzero(bad)[0]))
        if self.ld > self.cols:
            pad = self.bits[self.front:self.front + self.body].view(self.rows, self.ld)[:, self.cols:] != self.sentinel
            if bool(pad.any()):
                r, c = (int(v) for v in torch.nonzero(pad)[0])
                return ("pad", r, self.cols + c)
        bad = self.bits[self.front + self.body:] != self.sentinel
        if bool(bad.any()):
            return ("back", None, int(torch.nonzero(bad)[0]))
        return None

    def check(self, what: str = "") -> None:
        v = self.violation()
        if v is None:
            return
        region, r, c = v
        if region == "pad":
            where = f"pad column: row {r}, col {c} (extent {self.rows} x {self.cols}, ld {self.ld})"
        elif region == "back":
            where = (f"back guard: element {c} past the end = row {self.rows + c // self.ld}, col {c % self.ld} "
                     f"(extent {self.rows} x {self.cols}, ld {self.ld})")
        else:
            back = self.front - c
            where = f"front guard: {back} elements in front of the matrix = row {-((back + self.ld - 1) // self.ld)}, col {(-back) % self.ld}"
        raise AssertionError(f"{what}: written outside the described extent -- {where}")

    def untouched_interior(self) -> int:
        """how many interior elements still hold the sentinel (an output that every element of must be written: expect 0)"""
        return int((self.interior_bits() == self.sentinel).sum())
