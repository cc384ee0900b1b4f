"""A guarded arena for the tests: fp32 tensors that are views into one allocation each, laid out as
[front guard | tensor | back guard], so that a kernel's access outside a tensor lands in memory the test owns and
can be seen afterwards.

The three numbers of a guard's size (guard_bytes): at least GUARD_MIN = 64 KiB, and at least one image of the tensor
(its bytes / N, so that a store with a wrong image stride or one tile row too far still lands in a guard), capped at
GUARD_MAX = 64 MiB.

  * Arena.input(master): a copy of the master between guards filled with NaN (0 * NaN is NaN: a load past the end that
    is "masked" by a zero weight still poisons the result, which the parity assertions of the tests then see).  The
    CPU master is kept; check() compares the tensor with it bit for bit unless the case declares it in place.
  * Arena.output(*shape) / Arena.workspace(nbytes): NaN-filled, between guards filled with SENTINEL, a quiet-NaN bit
    pattern with a recognisable payload (a guard that leaks into arithmetic shows too).
  * Arena.check(tag): every guard still holds its fill bit for bit, every input still equals its master.

`align` is where the tensor starts: 256 puts it on a 256-byte boundary, 16 at an address that is 16 mod 256, the weakest
pointer winograd_mi355x.h accepts (WINO_E_ARG below 16).  Workspaces default to 256, the alignment the header asks for.

A plain module: the arena works on any torch device, the host tests (tests/test_guarded_host.py) use "cpu"."""
from __future__ import annotations

import collections

GUARD_MIN = 64 << 10
GUARD_MAX = 64 << 20
BOUNDARY = 256                 # `align` is an address modulo this
ALIGNS = (256, 16)             # the strongest and the weakest placement the sweeps run at
NAN_BITS = 0x7FC00000          # torch's float("nan")
SENTINEL = 0x7FC0DEAD          # quiet NaN, payload 0xDEAD
# workspaces that came through a passing check(), by the size query they were carved for (Arena.workspace(query=...))
WORKSPACE_RUNS = collections.Counter()


def guard_bytes(nbytes: int, images: int) -> int:
    """Bytes of each guard of a tensor of `nbytes` whose leading dimension is `images` (a multiple of BOUNDARY)."""
    image = -(-int(nbytes) // max(int(images), 1))
    g = min(max(GUARD_MIN, image), GUARD_MAX)
    return -(-g // BOUNDARY) * BOUNDARY


class GuardError(AssertionError):
    pass


class _Slot:
    def __init__(self, name, kind, buf, start, numel, shape, fill, master, in_place):
        self.name, self.kind, self.buf, self.start, self.numel = name, kind, buf, start, numel
        self.fill, self.master, self.in_place = fill, master, in_place
        self.tensor = buf[start:start + numel].view(shape)
        self.queries, self.counted = (), False

    def front(self):
        return self.buf[:self.start]

    def back(self):
        return self.buf[self.start + self.numel:]


class Arena:
    def __init__(self, torch, device, align: int = 256):
        self.torch, self.device, self.align = torch, torch.device(device), int(align)
        self.slots = []

    # ---- carving ------------------------------------------------------------------------------------------------
    def _carve(self, kind, shape, images, align, fill, name, master=None, in_place=False):
        torch = self.torch
        align = self.align if align is None else int(align)
        if align != BOUNDARY and (align <= 0 or align >= BOUNDARY or align % 4):
            raise ValueError(f"align must be {BOUNDARY} or a multiple of 4 below it, got {align}")
        shape = tuple(int(v) for v in shape)
        numel = 1
        for v in shape:
            numel *= v
        guard = guard_bytes(4 * numel, images)
        # room to slide the tensor to the wanted address without shortening either guard
        buf = torch.empty((2 * guard + 4 * numel + 2 * BOUNDARY) // 4, dtype=torch.float32, device=self.device)
        base = buf.data_ptr()
        assert base % 4 == 0
        start = guard + (align % BOUNDARY - (base + guard)) % BOUNDARY
        assert (base + start) % BOUNDARY == align % BOUNDARY and start % 4 == 0
        buf = buf[:(start + 4 * numel + guard) // 4]
        buf.view(torch.int32).fill_(fill)
        slot = _Slot(name or f"{kind}{len(self.slots)}", kind, buf, start // 4, numel, shape, fill, master, in_place)
        self.slots.append(slot)
        return slot

    def input(self, master, align=None, name=None, in_place=False):
        """A guarded copy of `master` (any device; its CPU copy is kept).  in_place: the case lets the library write
        it, so check() looks at its guards only."""
        m = master.detach().to("cpu").contiguous()
        if m.dtype != self.torch.float32:
            raise TypeError(f"the arena holds float32 tensors, got {m.dtype}")
        slot = self._carve("input", m.shape, m.shape[0] if m.dim() > 1 else 1, align, NAN_BITS, name, m, in_place)
        slot.tensor.copy_(m)
        return slot.tensor

    def output(self, *shape, align=None, name=None):
        slot = self._carve("output", shape, shape[0] if len(shape) > 1 else 1, align, SENTINEL, name)
        slot.tensor.fill_(float("nan"))
        return slot.tensor

    def workspace(self, nbytes: int, align: int = 256, name=None, query=()):
        """`nbytes` (rounded up to whole floats) as a flat NaN-filled tensor.  `query`: the name(s) of the size query
        that reported `nbytes`; a check() that passes counts the run in WORKSPACE_RUNS, once."""
        slot = self._carve("workspace", ((int(nbytes) + 3) // 4,), 1, align, SENTINEL, name)
        slot.queries = (query,) if isinstance(query, str) else tuple(query)
        slot.tensor.fill_(float("nan"))
        return slot.tensor

    # ---- checking -----------------------------------------------------------------------------------------------
    def _dirty(self):
        """Dirty words in all guards, and inputs that left their masters, as one number (one device round trip)."""
        torch = self.torch
        total = torch.zeros((), dtype=torch.int64, device=self.device)
        for s in self.slots:
            for g in (s.front(), s.back()):
                total += torch.count_nonzero(g.view(torch.int32) != s.fill)
            if s.master is not None and not s.in_place:
                total += torch.count_nonzero(s.tensor.view(torch.int32) != s.master.view(torch.int32).to(self.device))
        return int(total)

    def report(self):
        """One line per dirty guard or changed input."""
        torch = self.torch
        lines = []
        for s in self.slots:
            for side, g in (("front", s.front()), ("back", s.back())):
                bad = torch.nonzero(g.view(torch.int32) != s.fill).flatten()
                if bad.numel() == 0:
                    continue
                first, last = int(bad[0]) * 4, int(bad[-1]) * 4 + 3
                if side == "back":
                    where = (f"{last - first + 1} bytes written starting {first} bytes past the end "
                             f"(last dirty byte {last} past the end)")
                else:
                    n = g.numel() * 4
                    where = (f"{last - first + 1} bytes written starting {n - first} bytes before the start "
                             f"(last dirty byte {n - last} before the start)")
                lines.append(f"{s.name} ({s.kind}, {tuple(s.tensor.shape)}): {side} guard: {where}; "
                             f"{bad.numel()} dirty words")
            if s.master is not None and not s.in_place:
                bad = torch.nonzero(s.tensor.reshape(-1).view(torch.int32).cpu() != s.master.reshape(-1).view(torch.int32))
                bad = bad.flatten()
                if bad.numel():
                    lines.append(f"{s.name} (input, {tuple(s.tensor.shape)}): read-only operand written: "
                                 f"{bad.numel()} words differ from the master, first at byte {int(bad[0]) * 4}, "
                                 f"last at byte {int(bad[-1]) * 4 + 3}")
        return lines

    def check(self, tag: str = "") -> None:
        if self.device.type == "cuda":
            self.torch.cuda.synchronize(self.device)
        if self._dirty() == 0:
            for s in self.slots:
                if not s.counted:
                    s.counted = True
                    WORKSPACE_RUNS.update(s.queries)
            return
        raise GuardError(f"{tag}: " + "; ".join(self.report()))
