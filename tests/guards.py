"""Guard bands and poison around every tensor the Python layer allocates: the harness of the memory contract.

The contract: a kernel writes only inside its outputs and the first ``workspace_bytes`` of its workspace, and no result depends on
what an output or a workspace held before the call.  Every output and workspace of ``mcdseg`` comes from six torch allocators
(``torch.empty``, ``empty_like``, ``zeros``, ``zeros_like``, ``ones``, ``full_like``) and every workspace from ``ops._ws`` /
``ops._ws64``, so replacing those covers the library through the paths the trainers use::

    with guarded(device, interior=0xFF) as g:
        x = g.put(x_cpu)                  # inputs and in-place operands are guarded too
        y = ops.something(x)
        assert g.check() == []            # synchronises, then looks at every guard byte

A replaced allocation is a uint8 buffer ``guard | nbytes | guard``.  Both guards hold 0xA5; the interior holds ``interior`` (0xFF: a
NaN in every float type, -1 in every integer type) and then whatever the allocator promises (0, 1, the fill value).  The tensor handed
out is the interior viewed as the requested dtype and shape: contiguous, an autograd leaf like any fresh tensor, and -- ``guard`` being a
multiple of 512 -- as aligned as the caching allocator's own blocks, so the kernels' aligned paths run as in production.  The rear
guard starts at byte ``nbytes`` exactly: a float4 store past a ragged end, which the allocator's rounding to 512 B would swallow, lands in
it.  The registry holds every buffer until the context ends (a freed block cannot be inspected).

Out-of-bounds READS are not detectable this way and are not claimed; the poison catches only reads of unwritten memory INSIDE a buffer.
"""
import collections
import contextlib
import math

import torch

GUARD_BYTE = 0xA5
_ALLOCATORS = ("empty", "empty_like", "zeros", "zeros_like", "ones", "full_like")

Violation = collections.namedtuple("Violation", "kind shape dtype side first last")
Violation.__doc__ = """one violated allocation: ``kind`` the allocator, ``side`` "front" or "rear", ``first`` / ``last`` the byte offsets
of the first and last changed guard byte -- counted from the END of the tensor for the rear guard (0 is the first byte past the end) and
from its START for the front guard (-1 is the byte just before it)"""


def _device_of(d):
    d = torch.device(d) if d is not None else torch.get_default_device()
    if d.type == "cuda" and d.index is None:
        d = torch.device("cuda", torch.cuda.current_device())
    return d


def _size_of(args, kwargs):
    if "size" in kwargs:
        size = kwargs.pop("size")
    elif len(args) == 1 and not isinstance(args[0], int):
        size = args[0]
    else:
        size = args
    return tuple(int(s) for s in size)


class _Guarded:
    def __init__(self, device, interior, guard):
        if guard <= 0 or guard % 512:
            raise ValueError("the guard width must be a positive multiple of 512 bytes (the caching allocator's alignment), got %r" % (guard,))
        if not 0 <= int(interior) <= 0xFF:
            raise ValueError("the interior poison is one byte, got %r" % (interior,))
        self.device, self.interior, self.guard = _device_of(device), int(interior), int(guard)
        self.count = 0        # allocations intercepted (inputs moved with ``put`` included)
        self.workspaces = 0   # of which ``ops._ws`` / ``ops._ws64`` calls
        self._records = []    # (buffer, nbytes, kind, shape, dtype): strong references until the context ends
        self._real = {}

    # ------------------------------------------------------------------------------------------------ allocation
    def _launch_stream(self):
        """the stream the kernels that use a new block will run on when that is not torch's current one (ops._conv_backward puts a
        weight gradient on a side stream that has waited for the main one; the block comes from the main stream's pool as in
        production, but whatever fills it has to be ordered before those kernels)"""
        if self.device.type != "cuda":
            return None
        try:
            from mcdseg import ops
        except ImportError:
            return None
        return ops._LAUNCH.stream

    def _block(self, nbytes, kind, shape, dtype, fill=None):
        g = self.guard
        buf = self._real["empty"](g + nbytes + g, dtype=torch.uint8, device=self.device)
        side = self._launch_stream()
        with (torch.cuda.stream(side) if side is not None else contextlib.nullcontext()):
            buf[:g].fill_(GUARD_BYTE)
            buf[g + nbytes:].fill_(GUARD_BYTE)
            inner = buf[g:g + nbytes]
            inner.fill_(self.interior)
            t = inner.view(dtype).view(shape)
            if fill is not None:
                t.fill_(fill)
        self._records.append((buf, nbytes, kind, tuple(shape), dtype))
        self.count += 1
        return t

    def _new(self, kind, shape, dtype, fill=None, requires_grad=False):
        dtype = dtype if dtype is not None else torch.get_default_dtype()
        nbytes = math.prod(shape) * dtype.itemsize
        t = self._block(nbytes, kind, shape, dtype, fill)
        return t.requires_grad_(True) if requires_grad else t

    def _owns(self, device, kwargs):
        """this call is one the harness replaces: on its device, dense, contiguous, without ``out=`` / ``pin_memory`` or an option it
        does not know"""
        if _device_of(device) != self.device:
            return False
        if kwargs.get("out") is not None or kwargs.get("pin_memory"):
            return False
        if kwargs.get("layout", torch.strided) not in (None, torch.strided):
            return False
        if kwargs.get("memory_format", torch.contiguous_format) not in (None, torch.contiguous_format, torch.preserve_format):
            return False
        return not set(kwargs) - {"size", "dtype", "device", "requires_grad", "out", "pin_memory", "layout", "memory_format", "fill_value"}

    def _sized(self, kind, fill):
        real = self._real[kind]

        def alloc(*args, **kwargs):
            if not self._owns(kwargs.get("device"), kwargs) or kwargs.get("memory_format") is torch.preserve_format:
                return real(*args, **kwargs)
            try:
                shape = _size_of(args, dict(kwargs))
            except (TypeError, ValueError):
                return real(*args, **kwargs)
            return self._new(kind, shape, kwargs.get("dtype"), fill, bool(kwargs.get("requires_grad")))
        alloc.__name__ = kind
        return alloc

    def _like(self, kind, fill):
        real = self._real[kind]

        def alloc(ref, *args, **kwargs):
            value, given = fill, args
            if kind == "full_like":
                if args:
                    value, args = args[0], args[1:]
                else:
                    value = kwargs.get("fill_value")
            device = kwargs.get("device") if kwargs.get("device") is not None else getattr(ref, "device", None)
            own = torch.is_tensor(ref) and not args and self._owns(device, kwargs) and ref.layout == torch.strided
            if own and kwargs.get("memory_format", torch.preserve_format) in (None, torch.preserve_format):
                # preserve_format keeps the strides of a dense, permuted input (channels_last, a transpose): not the harness's business
                own = self._real["empty_like"](ref, device="meta").is_contiguous()
            if not own:
                return real(ref, *given, **kwargs)
            dtype = kwargs.get("dtype") if kwargs.get("dtype") is not None else ref.dtype
            return self._new(kind, tuple(ref.shape), dtype, value, bool(kwargs.get("requires_grad")))
        alloc.__name__ = kind
        return alloc

    def _ws(self, unit, dtype):
        def ws(nbytes, device):
            """a workspace of exactly ceil(nbytes / unit) elements: less than one element of slack, where the stock function adds one to
            two elements that would hide a one-element overrun"""
            n = -(-max(int(nbytes), 0) // unit)
            if _device_of(device) != self.device:
                return self._real["empty"](n, dtype=dtype, device=device)
            self.workspaces += 1
            return self._new("_ws" if unit == 4 else "_ws64", (n,), dtype)
        return ws

    def put(self, t, requires_grad=False):
        """a guarded copy of ``t`` (any device) on the harness's device: inputs and in-place operands"""
        t = t.detach()
        out = self._new("put", tuple(t.shape), t.dtype)
        out.copy_(t)
        return out.requires_grad_(True) if requires_grad else out

    # ------------------------------------------------------------------------------------------------ checking
    def check(self):
        """synchronise the device, then the list of ``Violation`` s: one per allocation and side whose guard bytes changed"""
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)
        if not self._records:
            return []
        g = self.guard
        flags = torch.stack([torch.stack(((buf[:g] != GUARD_BYTE).any(), (buf[g + nbytes:] != GUARD_BYTE).any()))
                             for buf, nbytes, _, _, _ in self._records]).cpu()
        found = []
        for (buf, nbytes, kind, shape, dtype), (front, rear) in zip(self._records, flags.tolist()):
            if front:
                at = (buf[:g] != GUARD_BYTE).nonzero().flatten()
                found.append(Violation(kind, shape, dtype, "front", int(at[0]) - g, int(at[-1]) - g))
            if rear:
                at = (buf[g + nbytes:] != GUARD_BYTE).nonzero().flatten()
                found.append(Violation(kind, shape, dtype, "rear", int(at[0]), int(at[-1])))
        return found

    # ------------------------------------------------------------------------------------------------ the context
    def __enter__(self):
        for kind in _ALLOCATORS:
            self._real[kind] = getattr(torch, kind)
        try:
            from mcdseg import ops
        except ImportError:
            ops = None
        self._ops = ops
        if ops is not None:
            self._real["_ws"], self._real["_ws64"] = ops._ws, ops._ws64
        fills = {"empty": None, "zeros": 0, "ones": 1, "empty_like": None, "zeros_like": 0, "full_like": None}
        for kind in _ALLOCATORS:
            setattr(torch, kind, (self._like if kind.endswith("_like") else self._sized)(kind, fills[kind]))
        if ops is not None:
            ops._ws, ops._ws64 = self._ws(4, torch.float32), self._ws(8, torch.float64)
        return self

    def __exit__(self, *exc):
        for kind in _ALLOCATORS:
            setattr(torch, kind, self._real[kind])
        if self._ops is not None:
            self._ops._ws, self._ops._ws64 = self._real["_ws"], self._real["_ws64"]
        if self.device.type == "cuda":
            torch.cuda.synchronize(self.device)  # nothing still writes into a buffer the registry is about to release
        self._records = []
        return False


def guarded(device, interior=0xFF, guard=1 << 16):
    """context manager: the six torch allocators and the workspace functions of ``mcdseg.ops`` give guarded, poisoned blocks on ``device``"""
    return _Guarded(device, interior, guard)
