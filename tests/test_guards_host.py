"""The guard-band harness itself (tests/guards.py), on CPU tensors: the patched allocators behave like torch's, what the harness does
not own is delegated, everything is restored, and an overrun of one element on either side is reported with its side and offset.  The
overruns are planted with torch indexing through ``as_strided`` on the registered buffer -- a plain torch function stands in for a
kernel; no kernel is made to overrun anywhere."""
import pytest
import torch

import guards
from guards import GUARD_BYTE, guarded

CPU = torch.device("cpu")
ALLOCATORS = [getattr(torch, k) for k in guards._ALLOCATORS]


def stray_write(t, element):
    """the stand-in for a faulty kernel: writes 1 into ``element`` of the flat tensor ``t``, which may lie before its start or past its
    end (inside the guard bands of the buffer the harness registered for it)"""
    flat = t.as_strided((1,), (1,), t.storage_offset() + element)
    flat.fill_(1)


def test_allocators_shape_dtype_values():
    with guarded(CPU) as g:
        a = torch.empty(3, 5, dtype=torch.float32)                  # varargs
        b = torch.empty((2, 3, 4), dtype=torch.int64, device="cpu")  # tuple
        c = torch.zeros(7, dtype=torch.float64)
        d = torch.ones((2, 2), dtype=torch.bfloat16)
        e = torch.full_like(a, 2.5)
        f = torch.zeros_like(b)
        h = torch.empty_like(a, dtype=torch.uint8)
        i = torch.empty(torch.Size((4, 1)))
        j = torch.empty(0)
        k = torch.full_like(b, fill_value=7)
        assert g.count == 10
        for t, shape, dtype in ((a, (3, 5), torch.float32), (b, (2, 3, 4), torch.int64), (c, (7,), torch.float64), (d, (2, 2), torch.bfloat16),
                                (e, (3, 5), torch.float32), (f, (2, 3, 4), torch.int64), (h, (3, 5), torch.uint8), (i, (4, 1), torch.float32),
                                (j, (0,), torch.float32), (k, (2, 3, 4), torch.int64)):
            assert tuple(t.shape) == shape and t.dtype == dtype and t.is_contiguous() and t.device == CPU
        assert torch.isnan(a).all() and bool((b == -1).all()) and bool((h == 0xFF).all())   # the 0xFF poison
        assert bool((c == 0).all()) and bool((d == 1).all()) and bool((e == 2.5).all()) and bool((f == 0).all()) and bool((k == 7).all())
        assert g.check() == []
    with guarded(CPU, interior=0x00) as g:
        assert bool((torch.empty(9) == 0).all()) and bool((torch.ones(3) == 1).all())


def test_alignment_is_kept():
    with guarded(CPU, guard=1024) as g:
        t = torch.empty(5, dtype=torch.float32)
        buf = g._records[0][0]
        assert t.data_ptr() == buf.data_ptr() + 1024 and buf.numel() == 2 * 1024 + 20   # the rear guard starts at byte nbytes exactly
        assert bool((buf[:1024] == GUARD_BYTE).all()) and bool((buf[1024 + 20:] == GUARD_BYTE).all())
    with pytest.raises(ValueError):
        guarded(CPU, guard=1000)


def test_requires_grad_and_backward_through_a_guarded_leaf():
    with guarded(CPU) as g:
        w = torch.zeros(4, 3, requires_grad=True)
        x = g.put(torch.arange(12.0).reshape(4, 3), requires_grad=True)
        e = torch.empty(2, 2, requires_grad=True)
        assert w.is_leaf and x.is_leaf and e.is_leaf and w.requires_grad and x.requires_grad and e.requires_grad
        ((w + 2.0) * x).sum().backward()
        assert torch.equal(w.grad, torch.arange(12.0).reshape(4, 3)) and torch.equal(x.grad, torch.full((4, 3), 2.0))
        with torch.no_grad():
            w.add_(1.0)   # an optimizer's in-place step on a guarded leaf
        assert bool((w == 1).all()) and g.check() == []


def test_foreign_calls_are_delegated():
    out = torch.empty(6)
    src = torch.empty(2, 3, 4, 5).to(memory_format=torch.channels_last)
    with guarded(CPU) as g:
        assert torch.zeros(6, out=out) is out
        t = torch.empty(2, 3, 4, 5, memory_format=torch.channels_last)
        assert t.is_contiguous(memory_format=torch.channels_last) and not t.is_contiguous()
        like = torch.empty_like(src)     # preserve_format of a permuted, dense tensor
        assert like.stride() == src.stride()
        assert torch.zeros(3, device="meta").device.type == "meta"
        assert torch.empty_like(out, device="meta").device.type == "meta"
        assert torch.empty(3, names=("n",)).names == ("n",)
        assert g.count == 0
        assert torch.empty_like(src, memory_format=torch.contiguous_format).is_contiguous() and g.count == 1
        assert torch.empty_like(out.expand(4, 6)).shape == (4, 6)


def test_everything_is_restored_also_after_an_exception():
    from mcdseg import ops
    ws, ws64 = ops._ws, ops._ws64
    with guarded(CPU):
        assert [getattr(torch, k) for k in guards._ALLOCATORS] != ALLOCATORS and ops._ws is not ws and ops._ws64 is not ws64
    assert [getattr(torch, k) for k in guards._ALLOCATORS] == ALLOCATORS and ops._ws is ws and ops._ws64 is ws64
    with pytest.raises(KeyError):
        with guarded(CPU):
            torch.empty(3)
            raise KeyError("inside")
    assert [getattr(torch, k) for k in guards._ALLOCATORS] == ALLOCATORS and ops._ws is ws and ops._ws64 is ws64


def test_workspaces_are_exact_and_counted():
    from mcdseg import ops
    with guarded(CPU) as g:
        assert ops._ws(17, CPU).numel() == 5 and ops._ws(16, CPU).numel() == 4 and ops._ws(0, CPU).numel() == 0
        assert ops._ws64(17, CPU).numel() == 3 and ops._ws64(16, CPU).dtype == torch.float64
        assert ops._ws(8, torch.device("meta")).device.type == "meta"
        assert g.workspaces == 5 and g.count == 5   # (the one on a foreign device is delegated, not counted)
    assert ops._ws(17, CPU).numel() == 5 and ops._ws(16, CPU).numel() == 5   # the stock function: 4 to 7 bytes of slack


# ---------------------------------------------------------------------------------------------------- sensitivity
@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.float64, torch.bfloat16])
def test_one_element_before_the_start_is_reported(dtype):
    with guarded(CPU) as g:
        torch.empty(4)
        t = torch.empty(3, 5, dtype=dtype)
        torch.zeros(2)
        t.fill_(1)
        assert g.check() == []                       # a clean run reports nothing
        stray_write(t, -1)
        found = g.check()
        assert len(found) == 1
        v = found[0]
        assert (v.kind, v.shape, v.dtype, v.side) == ("empty", (3, 5), dtype, "front")
        assert -dtype.itemsize <= v.first <= v.last <= -1   # inside the element just before the start (its bytes that are not 0xA5 already)


@pytest.mark.parametrize("dtype", [torch.float32, torch.uint8, torch.float64, torch.bfloat16])
def test_one_element_after_the_end_is_reported(dtype):
    with guarded(CPU) as g:
        t = torch.zeros(3, 5, dtype=dtype)
        u = torch.ones(7, dtype=dtype)
        assert g.check() == []
        stray_write(t, t.numel())
        found = g.check()
        assert len(found) == 1
        v = found[0]
        assert (v.kind, v.shape, v.dtype, v.side) == ("zeros", (3, 5), dtype, "rear")
        assert 0 <= v.first <= v.last <= dtype.itemsize - 1
        stray_write(u, u.numel() + 100)              # a second one, far into the band: both are named
        found = g.check()
        assert [(v.kind, v.side) for v in found] == [("zeros", "rear"), ("ones", "rear")]
        assert 100 * dtype.itemsize <= found[1].first <= found[1].last < 101 * dtype.itemsize


def test_a_whole_row_past_the_end_gives_first_and_last_offset():
    with guarded(CPU) as g:
        t = torch.empty(6, 10)
        t.as_strided((10,), (1,), t.storage_offset() + 60).fill_(0.0)
        (v,) = g.check()
        assert (v.side, v.first, v.last) == ("rear", 0, 39)


def test_a_write_three_bytes_past_a_workspace_is_caught():
    from mcdseg import ops
    with guarded(CPU) as g:
        ws = ops._ws(13, CPU)       # 4 floats: bytes 13..15 are the slack, byte 16 is the guard
        assert ws.numel() == 4 and g.check() == []
        byte = ws.view(torch.uint8)
        byte.as_strided((1,), (1,), byte.storage_offset() + 13 + 3).fill_(0)
        (v,) = g.check()
        assert (v.kind, v.shape, v.side, v.first, v.last) == ("_ws", (4,), "rear", 0, 0)


def test_put_guards_inputs_and_in_place_operands():
    with guarded(CPU) as g:
        src = torch.arange(10, dtype=torch.int64)
        x = g.put(src)
        assert torch.equal(x, src) and x.data_ptr() != src.data_ptr() and g.count == 1
        stray_write(x, 10)
        (v,) = g.check()
        assert (v.kind, v.side, v.first) == ("put", "rear", 0)
