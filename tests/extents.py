"""The arena of the memory-extent tests (tests/test_extents_cpu.py, tests/test_gpu_extents.py): a plain helper, no fixture.

An op's operands are laid into ONE uint8 buffer, each with a guard band in front of it and another behind it, and every byte that
is no operand element - the guards and the `ld - cols` gap behind every row - holds a filler.  After the op, verify() asserts bit
for bit that the filler and the inputs are as they were and that every output element was written.  Running the op on a tame
filler (1.0), on NaN and on +Inf and comparing the outputs bit for bit shows a read outside the operands that is multiplied away
instead of selected away: 0 * NaN is NaN.

Guard sizes are conditions, not measurements: 64 KiB in front; behind, 64 KiB and at least 256 rows of the operand's own row stride
(256 is the tallest tile in the tree).  Every buffer starts 256-byte aligned, as a fresh allocation would.

Outputs are pre-filled with "never written": a NaN of its own payload for the float types (the e4m3 code 0xFF for fp8), the most
negative value for the integer types - values no op of this library stores for the finite inputs the tests use.
Limitation: for int8 / uint8 the never-written value (0x80) is also the hostile filler's byte, and an output that legitimately holds
0x80 (int8 -128; the e4m3 code of -0 stored as uint8) or the e4m3 code 0xFF would be reported as never written.  The quantisers
here clamp to +-127 and the fp8 cast of finite input makes no NaN; a test of an op that can store those values must not use
role "out" for it.
"""
import torch

GUARD = 64 * 1024
TALLEST_TILE = 256
ALIGN = 256
FILLERS = ("tame", "nan", "inf")
F8 = getattr(torch, "float8_e4m3fn", None)
_INT_MIN = {torch.int8: -128, torch.int32: -2 ** 31, torch.int64: -2 ** 63}
_RAW = {1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}


def _is_f8(dt):
    return F8 is not None and dt == F8


def filler_value(dtype, filler):
    """the filler as a one-element tensor of `dtype` (fp8 and uint8 as their byte codes)"""
    if filler not in FILLERS:
        raise ValueError(f"filler must be one of {FILLERS}")
    if _is_f8(dtype):
        return torch.tensor([0x38 if filler == "tame" else 0x7F], dtype=torch.uint8).view(F8)      # 1.0 | NaN (e4m3 has no Inf)
    if dtype == torch.uint8:
        return torch.tensor([1 if filler == "tame" else 0x80], dtype=torch.uint8)
    if dtype in _INT_MIN:
        return torch.tensor([1 if filler == "tame" else _INT_MIN[dtype]], dtype=dtype)
    return torch.tensor([{"tame": 1.0, "nan": float("nan"), "inf": float("inf")}[filler]], dtype=dtype)


_NEVER = {torch.bfloat16: (torch.int16, 0x7FE1), torch.float16: (torch.int16, 0x7E01), torch.float32: (torch.int32, 0x7FE10000),
          torch.float64: (torch.int64, 0x7FFC200000000000)}


def unwritten_value(dtype):
    """a quiet NaN whose payload differs from the filler's and from any NaN arithmetic makes from it, so that a computed NaN is
    not mistaken for an element the op never wrote (e4m3 has one NaN per sign: the negative one)"""
    if _is_f8(dtype):
        return torch.tensor([0xFF], dtype=torch.uint8).view(F8)
    if dtype == torch.uint8:
        return torch.tensor([0x80], dtype=torch.uint8)
    if dtype in _INT_MIN:
        return torch.tensor([_INT_MIN[dtype]], dtype=dtype)
    raw, bits = _NEVER[dtype]
    return torch.tensor([bits], dtype=raw).view(dtype)


def _up(n, a):
    return -(-n // a) * a


class ExtentError(AssertionError):
    pass


class _Span:
    def __init__(self, name, col0, cols, role):
        self.name, self.col0, self.cols, self.role = name, col0, cols, role


class _Buffer:
    """one strided [rows, ld] buffer between its two guards, holding one operand or several side by side (column slices)"""
    def __init__(self, off, rows, ld, dtype, spans, front, back):
        self.off, self.rows, self.ld, self.dtype, self.spans, self.front, self.back = off, rows, ld, dtype, spans, front, back


class Arena:
    def __init__(self, device, filler="tame", capacity=48 << 20):
        if filler not in FILLERS:
            raise ValueError(f"filler must be one of {FILLERS}")
        self.device, self.filler = torch.device(device), filler
        self.buf = torch.zeros(capacity, dtype=torch.uint8, device=self.device)
        self.cur = 0
        self.buffers, self.shadow = [], None
        self.refused = False               # set by a case whose call must be refused: verify() then wants the outputs untouched too

    # ------------------------------------------------------------------ laying operands out
    def _typed(self, buf, off, n, dtype):
        item = torch.empty(0, dtype=dtype).element_size()
        return buf[off:off + n * item].view(dtype)

    def place(self, host, ld=None, role="in", name=None):
        """-> (device pointer, strided view [rows, cols]) of a copy of `host` ([..., cols], leading dimensions folded into rows)"""
        return self.place_fused([host], [role], pad=(0 if ld is None else ld - host.shape[-1]), names=[name])[0]

    def place_fused(self, hosts, roles, pad=0, names=None):
        """several operands of one dtype and one row count as column slices of one wider buffer, ld = sum(cols) + pad:
        -> [(pointer, view), ...].  What lies beside a slice in its rows is the other operands, then `pad` columns of filler."""
        hosts = [h.reshape(-1, h.shape[-1]) if h.dim() != 1 else h.reshape(1, -1) for h in hosts]
        dtype, rows = hosts[0].dtype, hosts[0].shape[0]
        if pad < 0 or any(h.dtype != dtype or h.shape[0] != rows for h in hosts) or any(r not in ("in", "out", "inout") for r in roles):
            raise ValueError("place: ld >= cols, one dtype and one row count per buffer, role in / out / inout")
        names = names or [None] * len(hosts)
        item = hosts[0].element_size()
        ld = sum(h.shape[1] for h in hosts) + pad
        front = _up(GUARD, ALIGN)
        back = _up(max(GUARD, TALLEST_TILE * ld * item), ALIGN)
        base = self.buf.data_ptr()
        off = _up(base + self.cur + front, ALIGN) - base
        front = off - self.cur
        end = _up(off + rows * ld * item + back, 8)                     # (whole elements of every dtype up to the next buffer)
        if end > self.buf.numel():
            raise ValueError(f"arena of {self.buf.numel()} bytes is too small: ask for a larger capacity")
        raw = filler_value(dtype, self.filler).view(_RAW[item])
        self.buf[self.cur:end].view(_RAW[item]).copy_(raw.to(self.device).expand((end - self.cur) // item))
        grid = self._typed(self.buf, off, rows * ld, dtype).view(rows, ld)
        spans, out, col = [], [], 0
        for h, role, nm in zip(hosts, roles, names):
            view = grid[:, col:col + h.shape[1]]
            if role == "out":
                view.view(_RAW[item]).copy_(unwritten_value(dtype).view(_RAW[item]).to(self.device).expand(rows, h.shape[1]))
            else:
                view.view(_RAW[item]).copy_(h.contiguous().view(_RAW[item]).to(self.device))
            spans.append(_Span(nm or f"operand{len(self.buffers)}.{len(spans)}", col, h.shape[1], role))
            out.append((self.buf.data_ptr() + off + col * item, view))
            col += h.shape[1]
        self.buffers.append(_Buffer(off, rows, ld, dtype, spans, front, back))
        self.cur = end
        self.shadow = None
        return out

    # ------------------------------------------------------------------ checking what the op did
    def arm(self):
        """remember the arena as it is now: call it after the last place() and before the op"""
        self.shadow = self.buf[:self.cur].clone()

    def _where(self, bad, b, base_elems):
        """first offending element of a flat mask -> (row, col) relative to the extent; base_elems: offset of mask[0] from the extent's start"""
        i = int(torch.nonzero(bad.reshape(-1))[0]) + base_elems
        return i // b.ld, i % b.ld

    def verify(self):
        """bit for bit: every filler byte and every `in` operand unchanged, no `out` element still never-written"""
        if self.shadow is None:
            raise RuntimeError("Arena.verify() without Arena.arm() after the last place()")
        now, then = self.buf[:self.cur], self.shadow
        for b in self.buffers:
            item = torch.empty(0, dtype=b.dtype).element_size()
            R = _RAW[item]
            names = " | ".join(s.name for s in b.spans)
            f0, n = b.off - b.front, b.rows * b.ld * item
            # guards are compared as bytes (the front one need not be a whole number of elements)
            bad = now[f0:b.off] != then[f0:b.off]
            if bool(bad.any()):
                k = -(-(b.front - int(torch.nonzero(bad)[-1])) // item)                             # elements before the start: the nearest one
                raise ExtentError(f"{names}: written in front of the operand, {k} element(s) before its start (row {(-k) // b.ld}, col {(-k) % b.ld})")
            bad = now[b.off + n:b.off + n + b.back] != then[b.off + n:b.off + n + b.back]
            if bool(bad.any()):
                e = int(torch.nonzero(bad)[0]) // item
                raise ExtentError(f"{names}: written behind the operand, row {b.rows + e // b.ld}, col {e % b.ld} (its extent is {b.rows} rows of {b.ld})")
            g_now = now[b.off:b.off + n].view(R).view(b.rows, b.ld)
            g_then = then[b.off:b.off + n].view(R).view(b.rows, b.ld)
            diff = g_now != g_then
            gap = torch.ones(b.ld, dtype=torch.bool, device=self.device)
            for s in b.spans:
                gap[s.col0:s.col0 + s.cols] = False
            bad = diff & gap[None, :]
            if bool(bad.any()):
                r, c = self._where(bad, b, 0)
                raise ExtentError(f"{names}: written in the gap between rows, row {r}, col {c} (rows are {b.ld} apart)")
            for s in b.spans:
                cols = slice(s.col0, s.col0 + s.cols)
                if s.role == "in":
                    bad = diff[:, cols]
                    if bool(bad.any()):
                        i = int(torch.nonzero(bad.reshape(-1))[0])
                        raise ExtentError(f"{s.name}: input modified at row {i // s.cols}, col {i % s.cols}")
                elif s.role == "out" and self.refused:
                    if bool(diff[:, cols].any()):
                        i = int(torch.nonzero(diff[:, cols].reshape(-1))[0])
                        raise ExtentError(f"{s.name}: output written by a refused call at row {i // s.cols}, col {i % s.cols}")
                elif s.role == "out":
                    never = unwritten_value(b.dtype).view(R).to(self.device)
                    bad = g_now[:, cols] == never
                    if bool(bad.any()):
                        i = int(torch.nonzero(bad.reshape(-1))[0])
                        raise ExtentError(f"{s.name}: output element never written at row {i // s.cols}, col {i % s.cols}")


def same_bits(a, b):
    """bit equality of two tensors of one dtype and shape (NaN payloads and signed zeros included)"""
    item = a.element_size()
    return a.shape == b.shape and a.dtype == b.dtype and bool(torch.equal(a.contiguous().view(_RAW[item]), b.contiguous().view(_RAW[item])))


def filler_passes(run, device, capacity=48 << 20, passes=("tame", "tame", "nan", "inf")):
    """run(arena) -> {name: output view} lays its operands into the arena, arms it, runs the op and returns the outputs.  One run
    per filler: the guards are verified after each, and the outputs of all runs must be bit-equal (the two tame runs are the
    control for run-to-run determinism).  -> the outputs of the first run, on the CPU."""
    results = []
    for filler in passes:
        arena = Arena(device, filler, capacity)
        outs = run(arena)
        if arena.device.type == "cuda":
            torch.cuda.synchronize()
        arena.verify()
        results.append({k: v.detach().cpu().clone() for k, v in outs.items()})
    first = results[0]
    for filler, res in list(zip(passes, results))[1:]:
        for k in first:
            if not same_bits(first[k], res[k]):
                d = first[k].contiguous().view(_RAW[first[k].element_size()]) != res[k].contiguous().view(_RAW[first[k].element_size()])
                i = int(torch.nonzero(d.reshape(-1))[0]); cols = first[k].shape[-1]
                what = "two runs on the tame filler differ (the op is not deterministic)" if filler == "tame" else f"the result depends on bytes outside the operands ({filler} filler)"
                raise ExtentError(f"{k}: {what}: first at row {i // cols}, col {i % cols}, {int(d.sum())} element(s)")
    return first
