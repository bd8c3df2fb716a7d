"""GPU: the memory contract of every kernel ("The memory contract"), through the paths the trainers use.

A kernel writes only inside its outputs and the first ``workspace_bytes`` of its workspace, and no result depends on what an output or
a workspace held before the call.  ``hold(workload)`` runs one operation three times -- under the stock allocator, under
``guards.guarded(interior=0xFF)`` (NaN in every float type, -1 in the integer types) and under ``guarded(interior=0x00)`` -- and asserts
that no guard byte changed and that every returned tensor is bit for bit the same in the three runs.  Every kernel is bitwise
reproducible (no float atomics), so there is no tolerance to choose.  Each case is one operation at the smallest shape at which its
kernel has a ragged end: a channel count padded to the tile, a pixel count that is no multiple of the vector width, a last partial row."""
import ctypes

import pytest
import torch

from guards import guarded

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------------- the helper
class _Stock:
    """the first run: plain tensors from the caching allocator"""

    def __init__(self, device):
        self.device = device

    def put(self, t, requires_grad=False):
        out = t.detach().to(self.device)
        return out.requires_grad_(True) if requires_grad else out


def _bits(t):
    """the tensor as integers of its element size: NaNs compare by bit pattern"""
    t = t.detach().contiguous()
    if t.dtype.is_floating_point:
        t = t.view({2: torch.int16, 4: torch.int32, 8: torch.int64}[t.dtype.itemsize])
    return t


def hold(device, workload, workspace=False, family=None):
    """``workload(put)`` builds its inputs on the CPU from a seeded generator, moves them with ``put`` and returns a dict of named
    tensors.  ``workspace``: the operation has a ``*_workspace_bytes`` function, so at least one workspace must have been intercepted."""
    from mcdseg import ops
    ops._PACK_TABLES.clear()
    ref = {k: v.detach().clone() for k, v in workload(_Stock(device).put).items()}
    torch.cuda.synchronize(device)
    assert ref, "the workload returns nothing"
    seen = []
    for interior in (0xFF, 0x00):
        with guarded(device, interior=interior) as g:
            ops._PACK_TABLES.clear()   # no device table cached by an earlier run escapes the guards (nor does one of this run survive it)
            try:
                out = workload(g.put)
                found = g.check()
                got = {k: v.detach().clone() for k, v in out.items()}
            finally:
                ops._PACK_TABLES.clear()
            count, workspaces = g.count, g.workspaces
        assert found == [], "poison 0x%02X: a kernel wrote outside its memory: %s" % (interior, found)
        assert sorted(got) == sorted(ref)
        for k in ref:
            assert got[k].shape == ref[k].shape and got[k].dtype == ref[k].dtype, k
            same = torch.equal(_bits(got[k]), _bits(ref[k]))
            if not same:
                diff = (_bits(got[k]) != _bits(ref[k])).flatten().nonzero().flatten()
                raise AssertionError("poison 0x%02X: %s depends on what its memory held before: %d of %d elements differ, the first at %d, the last at %d"
                                     % (interior, k, diff.numel(), ref[k].numel(), int(diff[0]), int(diff[-1])))
        assert count >= len(ref), "the workload allocated %d tensors through the harness for %d outputs: it bypassed it" % (count, len(ref))
        assert not workspace or workspaces >= 1, "no workspace was intercepted"
        seen.append((count, workspaces))
    assert seen[0] == seen[1], "the two guarded runs allocated differently: %s" % (seen,)
    print("memory contract [%s]: %d guarded allocations, %d workspaces" % (family or workload.__name__, seen[0][0], seen[0][1]))
    return ref


class _Names:
    """``ops.LAUNCH_TIMER`` that only records which kernels were named (test_kernels_gpu.py's idiom)"""

    def __init__(self):
        self.names = []

    def wants(self, name):
        self.names.append(name)
        return False


class named:
    def __enter__(self):
        from mcdseg import ops
        self.prev, self.rec = ops.LAUNCH_TIMER, _Names()
        ops.LAUNCH_TIMER = self.rec
        return self.rec.names

    def __exit__(self, *exc):
        from mcdseg import ops
        ops.LAUNCH_TIMER = self.prev


def place(module, put):
    """``module.to(device)`` through ``put``: every parameter and buffer (the running statistics are in-place operands) is guarded"""
    for m in module.modules():
        for p in m._parameters.values():
            if p is not None:
                p.data = put(p.data)
        for k, b in list(m._buffers.items()):
            if b is not None:
                m._buffers[k] = put(b)
    return module


def _randn(g, *shape):
    return torch.randn(*shape, generator=g)


# ---------------------------------------------------------------------------------------------------- convolution groups
# (Cin, Cout, k, stride, dil, H, W, N, bias)
GROUP_CASES = [
    (6, 16, 7, 1, 1, 20, 28, 2, False),     # the stem, K padded
    (1, 16, 7, 1, 1, 9, 13, 2, False),
    (16, 16, 3, 1, 1, 21, 45, 2, False),    # the thin layers' window kernels
    (16, 32, 3, 2, 1, 21, 27, 2, False),
    (32, 64, 1, 2, 1, 20, 28, 2, False),
    (64, 128, 3, 2, 1, 13, 19, 3, False),
    (128, 256, 3, 1, 2, 12, 15, 2, False),
    (512, 41, 1, 1, 1, 8, 12, 2, True),     # M padded 41 -> 64
    (40, 24, 3, 1, 1, 11, 13, 2, True),
]


def _group(case, seed=11):
    from models.drn import BatchNorm2d, Conv2d
    cin, cout, k, s, d, h, w, n, bias = case
    g = torch.Generator().manual_seed(seed)
    pad = d * (k // 2)
    conv, bn = Conv2d(cin, cout, k, stride=s, padding=pad, dilation=d, bias=bias), BatchNorm2d(cout)
    with torch.no_grad():
        conv.weight.copy_(_randn(g, *conv.weight.shape) * (2.0 / (k * k * cout)) ** 0.5)
        if bias:
            conv.bias.copy_(_randn(g, cout))
        bn.weight.copy_(1 + 0.2 * _randn(g, cout)), bn.bias.copy_(0.1 * _randn(g, cout))
        bn.running_mean.copy_(0.05 * _randn(g, cout)), bn.running_var.copy_(1 + 0.1 * torch.rand(cout, generator=g))
    x = _randn(g, n, cin, h, w) + 0.3
    ho, wo = (h + 2 * pad - d * (k - 1) - 1) // s + 1, (w + 2 * pad - d * (k - 1) - 1) // s + 1
    return conv, bn, x, _randn(g, n, cout, ho, wo)


@pytest.mark.parametrize("math", ["f32", "bf16x6", "f16x3", "f16x1"])
@pytest.mark.parametrize("case", GROUP_CASES, ids=lambda c: "x".join(map(str, c[:8])))
def test_conv_group_forward_and_backward(case, math, device, monkeypatch):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)

    def group(put):
        conv, bn, x, gy = _group(case)
        place(conv, put), place(bn, put).train()
        xg = put(x, requires_grad=True)
        y = ops.conv_bn_act(xg, conv, bn, relu=True)
        y.backward(put(gy))
        out = dict(y=y, dx=xg.grad, dw=conv.weight.grad, dgamma=bn.weight.grad, dbeta=bn.bias.grad, running_mean=bn.running_mean,
                   running_var=bn.running_var, num_batches_tracked=bn.num_batches_tracked)
        if conv.bias is not None:
            out["dbias"] = conv.bias.grad
        return out
    hold(device, group, workspace=True, family="conv group %s" % math)


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("case", [GROUP_CASES[0], GROUP_CASES[5], GROUP_CASES[7], GROUP_CASES[8]], ids=lambda c: "x".join(map(str, c[:8])))
def test_conv_group_other_forms(case, math, device, monkeypatch):
    """the same groups with a residual and without ReLU, with eval-mode statistics on a tape, folded for inference, and the
    convolution with bias alone (the 1x1 ``seg`` head)"""
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)

    def forms(put):
        out = {}
        for form in ("residual", "linear", "eval", "folded", "bias-only"):
            conv, bn, x, gy = _group(case)
            place(conv, put), place(bn, put).train(form not in ("eval", "folded"))
            xg, res = put(x, requires_grad=form != "folded"), put(0.5 * gy, requires_grad=form == "residual")
            if form == "folded":
                with torch.no_grad():
                    out["folded/y"] = ops.conv_bn_act(xg, conv, bn, relu=True, residual=res)
                continue
            if form == "bias-only":
                if conv.bias is None:
                    continue
                y = ops.conv2d_bias(xg, conv)
            else:
                y = ops.conv_bn_act(xg, conv, bn, relu=form != "linear", residual=res if form == "residual" else None)
            y.backward(put(gy))
            out.update({form + "/y": y, form + "/dx": xg.grad, form + "/dw": conv.weight.grad, form + "/running_var": bn.running_var})
            if form != "bias-only":
                out.update({form + "/dgamma": bn.weight.grad, form + "/dbeta": bn.bias.grad})
            if form == "residual":
                out["residual/dres"] = res.grad
            if conv.bias is not None:
                out[form + "/dbias"] = conv.bias.grad
        return out
    hold(device, forms, workspace=True, family="conv group forms %s" % math)


def _block_workload(kind, planes, stride, hw, n, storage, trunk):
    """a residual block behind one plain group (so that its input carries a companion), inside ``late_weight_grads``: the weight
    gradients of the groups with companions run on the side stream, as in a trainer's trunk"""
    from mcdseg import ops
    from models import drn

    def block(put):
        g = torch.Generator().manual_seed(15)
        cls = drn.BasicBlock if kind == "basic" else drn.Bottleneck
        inpl = planes * cls.expansion if stride == 1 else planes // 2
        outpl = planes * cls.expansion
        torch.manual_seed(4)
        down = None
        if stride != 1 or inpl != outpl:
            down = drn.ConvBN(drn.Conv2d(inpl, outpl, kernel_size=1, stride=stride, bias=False), drn.BatchNorm2d(outpl))
        mods = torch.nn.ModuleList([drn.ConvBNReLU(drn.Conv2d(inpl, inpl, 3, padding=1, bias=False), drn.BatchNorm2d(inpl), torch.nn.ReLU(inplace=True)),
                                    cls(inpl, planes, stride, down, dilation=(1, 1)),
                                    drn.ConvBNReLU(drn.Conv2d(outpl, 24, 3, padding=1, bias=False), drn.BatchNorm2d(24), torch.nn.ReLU(inplace=True))])
        place(mods, put).train()
        x = put(_randn(g, n, inpl, *hw), requires_grad=True)
        with ops.late_weight_grads(mods):
            if trunk:
                with ops.trunk_internal():
                    h = mods[1](mods[0](x))
                    virtual = ops.is_virtual(h)
            else:
                h, virtual = mods[1](mods[0](x)), False
            y = mods[2](h)
            assert virtual == (storage == "compact")
        y.backward(put(_randn(g, *y.shape)))
        out = dict(y=y, dx=x.grad)
        for i, p in enumerate(mods.parameters()):
            out["grad%d" % i] = p.grad
        for i, b in enumerate(m for m in mods.modules() if isinstance(m, drn.BatchNorm2d)):
            out["running_var%d" % i] = b.running_var
        return out
    return block


def test_basic_block_with_the_relu_bit_plane(device, monkeypatch):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    monkeypatch.setattr(ops, "RELU_MASK", True)
    hold(device, _block_workload("basic", 128, 2, (28, 40), 2, "fp32", False), workspace=True, family="BasicBlock, bit-plane")


@pytest.mark.parametrize("math,storage", [("f16x3", "compact"), ("f16x1", "compact"), ("f16x3", "fp32")], ids=["compact", "two-byte", "fp32"])
def test_bottleneck_in_each_storage(math, storage, device, monkeypatch):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)
    monkeypatch.setattr(ops, "ACT_STORAGE", storage)
    monkeypatch.setattr(ops, "HALF_STORAGE", True)
    hold(device, _block_workload("bottleneck", 64, 1, (11, 13), 2, storage, storage == "compact"), workspace=True, family="Bottleneck %s %s" % (math, storage))


def test_conv_batch_split_under_a_small_launch_limit(device, monkeypatch):
    """``test_conv_batch_split_for_large_operands``' geometry: the second group's three passes run in slices of 2, 2 and 1 images, from
    the companions -- asserted by kernel name as that test asserts it"""
    from mcdseg import ops
    from models.drn import BatchNorm2d, Conv2d
    monkeypatch.setattr(ops, "MAX_CONV_BYTES", 2 * 4 * 136 * 12 * 14)
    assert ops._batch_pieces(ops.conv_desc((5, 40, 12, 14), (136, 40, 3, 3), 1, 1, 1)) == [(0, 2), (2, 4), (4, 5)]

    seen = []

    def split(put):
        g = torch.Generator().manual_seed(2)
        torch.manual_seed(2)
        mods = torch.nn.ModuleList([Conv2d(24, 40, 3, padding=2, dilation=2, bias=False), BatchNorm2d(40), Conv2d(40, 136, 3, padding=1, bias=False), BatchNorm2d(136)])
        place(mods, put).train()
        x = put(_randn(g, 5, 24, 12, 14), requires_grad=True)
        gy = put(_randn(g, 5, 136, 12, 14))
        with named() as names:
            y = ops.conv_bn_act(ops.conv_bn_act(x, mods[0], mods[1], relu=True), mods[2], mods[3], relu=True)
            y.backward(gy)
        seen.append(list(names))
        out = dict(y=y, dx=x.grad, running_var1=mods[1].running_var, running_var2=mods[3].running_var)
        for i, p in enumerate(mods.parameters()):
            out["grad%d" % i] = p.grad
        return out
    hold(device, split, workspace=True, family="conv batch split")
    assert len(seen) == 3
    for names in seen:  # the second group's three passes ran from the companions, slice by slice
        pre = [nm for nm in names if (nm.startswith("conv_gemm_split_kernel") and nm.endswith("true>")) or nm.startswith("conv_gemm_split_pp_kernel")]
        assert len(pre) >= 6, names
        assert sum(nm.startswith("conv_wgrad_split_tr") for nm in names) >= 3, names


# ---------------------------------------------------------------------------------------------------- BatchNorm alone
@pytest.mark.parametrize("one", [1024, 0], ids=["one-launch", "two-stage"])
@pytest.mark.parametrize("rows,c,mp", [(7, 16, 32), (333, 24, 32), (1000, 41, 64)])
def test_bn_statistics(rows, c, mp, one, device, libopt):
    from mcdseg import ops
    libopt(BN_STATS_ONE=one)
    L = ops.lib()

    def stats(put):
        g = torch.Generator().manual_seed(rows * 131 + c)
        part = torch.zeros(rows, 3, mp)
        part[:, 0, :c] = torch.randint(1, 161, (rows, 1), generator=g).float()
        part[:, 1, :c] = _randn(g, rows, c) * 3.0 + 1.5
        part[:, 2, :c] = torch.rand(rows, c, generator=g) * 100.0
        part, gam, bet = put(part), put(_randn(g, c)), put(_randn(g, c))
        resb, rm, rv = put(torch.tensor([2.75])), put(torch.full((c,), 0.25)), put(torch.full((c,), 1.5))
        nbt = put(torch.full((1,), 5, dtype=torch.int64))
        mean, rstd, yb = torch.empty(c, device=device), torch.empty(c, device=device), torch.empty(1, device=device)
        ws = ops._ws64(L.mcdseg_bn_stats_workspace_bytes(rows, c), device)
        ops.check(L.mcdseg_bn_stats_finalize(ops._p(part), rows, c, mp, ops._p(mean), ops._p(rstd), ops._p(rm), ops._p(rv), ops._p(nbt), 0.1, 1e-5,
                                             ops._p(gam), ops._p(bet), ops._p(resb), ops._p(yb), 2, ops._p(ws), ctypes.c_size_t(ws.numel() * 8),
                                             ops._stream()), "bn_stats_finalize")
        return dict(mean=mean, rstd=rstd, running_mean=rm, running_var=rv, num_batches_tracked=nbt, y_bound=yb)
    hold(device, stats, workspace=True, family="BatchNorm statistics")


@pytest.mark.parametrize("shape", [(2, 41, 9, 11), (3, 16, 6, 10)], ids=lambda s: "x".join(map(str, s)))
def test_bn_apply_and_backward_with_each_mask_source(shape, device, monkeypatch):
    """the BatchNorm entry points alone (test_bn_contract_gpu.py's wrappers, whose tensors come from the patched allocators): apply, the
    backward reduce and apply with the mask from y, from z, and without ReLU at both shapes; the mask from the companion's sign and from the
    bit-plane at (3, 16, 6, 10) only -- their entry points take C % 8 == 0 and HW % 4 == 0, which (2, 41, 9, 11) is not"""
    import test_bn_contract_gpu as B
    from mcdseg import ops
    L = ops.lib()
    n, c, h, w = shape
    monkeypatch.setattr(B, "_bwd_ws", lambda s, dev: ops._ws(L.mcdseg_bn_bwd_workspace_bytes(s[0], s[1], s[2] * s[3]), dev))
    cb_ok = c % 8 == 0 and (h * w) % 4 == 0

    def bn(put):
        g = torch.Generator().manual_seed(77)
        z, dy, res = put(_randn(g, *shape) + 0.3), put(_randn(g, *shape)), put(_randn(g, *shape))
        zc = z.double().cpu()
        mean, var = zc.mean((0, 2, 3)), zc.var((0, 2, 3), unbiased=False)
        mean, rstd = put(mean.float()), put((1.0 / torch.sqrt(var + 1e-5)).float())
        gamma, beta = put(1 + 0.2 * _randn(g, c)), put(0.1 * _randn(g, c))
        out = {}
        for relu in (False, True):
            tag = "relu" if relu else "linear"
            y = B._k_apply(z, mean, rstd, gamma, beta, res, relu)
            dgamma, dbeta, db = B._k_reduce(dy, y, z, mean, rstd, gamma, relu, True, want_bound=True)
            dz, dres = B._k_bwd_apply(dy, y, z, mean, rstd, gamma, dgamma, dbeta, relu, True, True)
            out.update({tag + "/y": y, tag + "/dgamma": dgamma, tag + "/dbeta": dbeta, tag + "/dz_bound": db, tag + "/dz": dz, tag + "/dres": dres})
        y0 = B._k_apply(z, mean, rstd, gamma, beta, None, True)
        dgamma, dbeta, db = B._k_reduce_zmask(dy, z, mean, rstd, gamma, beta, True)
        out.update({"z/y": y0, "z/dgamma": dgamma, "z/dbeta": dbeta, "z/dz_bound": db})
        if cb_ok:
            bound = ops.absmax(z) * 0 + 64.0
            dbound = ops.absmax(dy)
            y, cb = B._k_apply_cb(z, mean, rstd, gamma, beta, res, True, bound, B.F16X3)
            dg, dbt, _ = B._k_reduce(dy, None, z, mean, rstd, gamma, True, True, y_cb=cb, math_id=B.F16X3)
            dz, dres, dcb = B._k_bwd_apply_cb(dy, None, cb, z, mean, rstd, gamma, dg, dbt, dbound, B.F16X3, True, True)
            out.update({"y_cb/y": y, "y_cb/unsplit": B._k_unsplit(cb, bound, B.F16X3, z), "y_cb/dgamma": dg, "y_cb/dz": dz, "y_cb/dres": dres,
                        "y_cb/dz_unsplit": B._k_unsplit(dcb, dbound, B.F16X3, z)})
            dz, dcb = B._k_bwd_apply_cb_zmask(dy, z, mean, rstd, gamma, beta, dgamma, dbeta, dbound, B.F16X3, True)
            out.update({"z/dz": dz, "z/dz_unsplit": B._k_unsplit(dcb, dbound, B.F16X3, z)})
            y, cb, rmask = B._k_apply_cb_mask(z, mean, rstd, gamma, beta, res, bound, B.F16X3)
            dg, dbt, db = B._k_reduce_mask(dy, rmask, z, mean, rstd, gamma, True)
            dz, dres, dcb = B._k_bwd_apply_cb_mask(dy, rmask, z, mean, rstd, gamma, dg, dbt, dbound, B.F16X3, True)
            out.update({"bits/y": y, "bits/dgamma": dg, "bits/dbeta": dbt, "bits/dz_bound": db, "bits/dz": dz, "bits/dres": dres,
                        "bits/dz_unsplit": B._k_unsplit(dcb, dbound, B.F16X3, z)})
        return out
    hold(device, bn, workspace=True, family="BatchNorm apply/backward")


def test_bn_two_byte_backward_reduce(device):
    """``mcdseg_bn_bwd_reduce_half`` at (2, 256, 11, 13) on 16-bit unit images, linear and with the mask from the activation's sign, train
    and eval (the apply kernels of the 2-byte chain run at this very shape inside ``test_bottleneck_in_each_storage[two-byte]``)"""
    from mcdseg import ops
    from test_half_storage_gpu import _nchw_to_units, _scale
    L = ops.lib()
    n, c, h, w = 2, 256, 11, 13

    def half(put):
        g = torch.Generator().manual_seed(78)
        z, dy, y = _randn(g, n, c, h, w) + 0.3, _randn(g, n, c, h, w), _randn(g, n, c, h, w)
        z_bound = (z.abs().max() * 37.0).reshape(1)
        z16 = put(_nchw_to_units((z / _scale(z_bound)).to(torch.float16)))
        dy16, y16 = put(_nchw_to_units(dy.to(torch.bfloat16))), put(_nchw_to_units((y / 8).to(torch.float16)))
        mean = put(z.mean((0, 2, 3)))
        rstd = put(1.0 / torch.sqrt(z.var((0, 2, 3), unbiased=False) + 1e-5))
        gamma, beta, zb = put(1 + 0.2 * _randn(g, c)), put(0.1 * _randn(g, c)), put(z_bound)
        out = {}
        for kind in (0, 4):
            for train in (1, 0):
                dgamma, dbeta, db = torch.empty(c, device=device), torch.empty(c, device=device), torch.empty(1, device=device)
                ws = ops._ws(L.mcdseg_bn_bwd_half_workspace_bytes(n, c, h * w), device)
                ops.check(L.mcdseg_bn_bwd_reduce_half(ops._p(dy16), ops._p(y16) if kind == 4 else None, ops._p(z16), ops._p(zb), ops._p(mean), ops._p(rstd),
                                                      ops._p(gamma), ops._p(beta), ops._p(dgamma), ops._p(dbeta), ops._p(db), kind, train, n, c, h * w,
                                                      ops._p(ws), ctypes.c_size_t(ws.numel() * 4), ops._stream()), "bn_bwd_reduce_half")
                out.update({"dgamma/%d/%d" % (kind, train): dgamma, "dbeta/%d/%d" % (kind, train): dbeta, "dz_bound/%d/%d" % (kind, train): db})
        return out
    hold(device, half, workspace=True, family="BatchNorm 2-byte reduce")


# ---------------------------------------------------------------------------------------------------- heads and losses
@pytest.mark.parametrize("shape", [(1, 5, 3, 7), (2, 41, 8, 12)], ids=lambda s: "x".join(map(str, s)))
def test_up8_forward_and_backward(shape, device):
    from mcdseg import ops
    n, c, hi, wi = shape

    def up8(put):
        g = torch.Generator().manual_seed(5)
        x, w = put(_randn(g, n, c, hi, wi), requires_grad=True), put(_randn(g, c, 1, 16, 16) * 0.1, requires_grad=True)
        x2, w2 = put(_randn(g, n, c, hi, wi), requires_grad=True), put(_randn(g, c, 1, 16, 16) * 0.1, requires_grad=True)
        gy = put(_randn(g, n, c, 8 * hi, 8 * wi))
        y = ops.up8(x, w)
        y.backward(gy)
        y2 = ops.up8_dual(x, w, x2, w2)
        dxi, dwi = ops._up8_bwd_input(gy, w.detach(), n, c, hi, wi), ops._up8_bwd_weight(gy, x.detach(), n, c, hi, wi)
        return dict(y=y, dx=x.grad, dw=w.grad, dual=y2, dx_separate=dxi, dw_separate=dwi)
    hold(device, up8, workspace=True, family="up8")


@pytest.mark.parametrize("shape", [(2, 4, 1, 1), (1, 1, 4, 200)], ids=lambda s: "x".join(map(str, s)))
def test_up8_backward_band_kernel(shape, device):
    from mcdseg import ops
    n, c, hi, wi = shape

    def band(put):
        g = torch.Generator().manual_seed(6)
        x, w, gy = put(_randn(g, n, c, hi, wi)), put(_randn(g, c, 1, 16, 16) * 0.1), put(_randn(g, n, c, 8 * hi, 8 * wi))
        dx, dw = ops._up8_bwd(gy, w, x, True, True)
        dx1, _ = ops._up8_bwd(gy, w, x, True, False)
        _, dw1 = ops._up8_bwd(gy, w, x, False, True)
        return dict(dx=dx, dw=dw, dx_alone=dx1, dw_alone=dw1)
    hold(device, band, workspace=True, family="up8 band")


@pytest.mark.parametrize("dma", [1, 0])
@pytest.mark.parametrize("mode", ["ce+diff", "diff", "ce-single", "shared-scores"])
@pytest.mark.parametrize("shape", [(2, 41, 5, 7), (1, 12, 3, 20)], ids=lambda s: "x".join(map(str, s)))
def test_up8_loss_fused(shape, mode, dma, device, libopt):
    from mcdseg import ops
    libopt(UP8_LOSS_DMA=dma)
    assert ("_dma_" in ops.up8_loss_kernel_name(*shape, mode != "ce-single", mode != "diff")) == (dma == 1)
    n, c, hi, wi = shape
    single = mode == "ce-single"

    def fused(put):
        g = torch.Generator().manual_seed(11)
        s1 = put(2 * _randn(g, n, c, hi, wi))
        s2 = s1 if mode == "shared-scores" else put(2 * _randn(g, n, c, hi, wi))
        w1, w2 = put(_randn(g, c, 1, 16, 16) * 0.2), put(_randn(g, c, 1, 16, 16) * 0.2)
        lab = torch.randint(0, c, (n, 8 * hi, 8 * wi), generator=g)
        lab[0, 0, :5] = -100
        lab, cw = put(lab), put(0.5 + torch.rand(c, generator=g))
        kw = dict(ce_coef=0.0 if mode == "diff" else 1.0, diff_coef=0.0 if single else 0.7)
        labels = None if mode == "diff" else lab
        with named() as names:
            losses, g1, g2 = ops.up8_mcd_losses(s1, w1, None if single else s2, None if single else w2, labels, cw if labels is not None else None, **kw)
        assert any(("_dma_" in nm) == (dma == 1) for nm in names if nm.startswith("up8_softmax")), names
        vals, _, _ = ops.up8_mcd_losses(s1, w1, None if single else s2, None if single else w2, labels, cw if labels is not None else None,
                                        want_grad=False, **kw)
        out = dict(losses=losses, g1=g1, values_only=vals)
        if not single:
            out["g2"] = g2
        return out
    hold(device, fused, workspace=True, family="up8+loss")


@pytest.mark.parametrize("c", [3, 14, 41, 48])
@pytest.mark.parametrize("dist", ["diff", "jsd", "symkl", "mis_symkl"])
def test_mcd_losses(dist, c, device):
    from mcdseg import ops

    def losses(put):
        g = torch.Generator().manual_seed(100 + c)
        z1, z2 = put(2 * _randn(g, 2, c, 9, 13)), put(2 * _randn(g, 2, c, 9, 13))
        lab = torch.randint(0, c, (2, 9, 13), generator=g)
        lab[1, 2, :4] = -100
        lab, cw = put(lab), put(0.5 + torch.rand(c, generator=g))
        l, g1, g2 = ops.mcd_losses(z1, z2, lab, cw, ce_coef=1.0, diff_coef=0.7, dist=dist)
        v, _, _ = ops.mcd_losses(z1, z2, lab, cw, ce_coef=1.0, diff_coef=0.7, want_grad=False, dist=dist)
        out = dict(losses=l, g1=g1, g2=g2, values_only=v, wsum=ops.label_weight_sum(lab, cw, c))
        if dist == "diff":
            l1, h1, _ = ops.mcd_losses(z1, None, lab, cw, ce_coef=1.0)
            out.update(single=l1, single_g=h1)
        return out
    hold(device, losses, workspace=True, family="mcd_losses")


def test_predict_tails(device):
    from mcdseg import ops

    def tails(put):
        g = torch.Generator().manual_seed(31)
        z1, z2 = put(2 * _randn(g, 2, 41, 7, 9)), put(2 * _randn(g, 2, 41, 7, 9))
        s, w = put(2 * _randn(g, 2, 41, 3, 5)), put(_randn(g, 41, 1, 16, 16) * 0.2)
        lab, ent = ops.predict_labels(z1, z2, 40)
        lab1, ent1 = ops.predict_labels(z1, None, 41)
        labu, entu = ops.predict_labels_up8(s, w, 40)
        labb, entb = ops.predict_labels_bilinear8(s, 41)
        return dict(labels=lab, entropy=ent, labels1=lab1, entropy1=ent1, labels_up8=labu, entropy_up8=entu, labels_bilinear8=labb, entropy_bilinear8=entb,
                    depth=ops.depth_image_u8(put(_randn(g, 2, 1, 3, 5))), depth3=ops.depth_image_u8(put(_randn(g, 1, 3, 2, 7))))
    hold(device, tails, workspace=True, family="predict tails")


@pytest.mark.parametrize("cmid,groups", [(10, 1), (10, 2), (1, 2)])
def test_dann_down(cmid, groups, device):
    from mcdseg import ops

    def down(put):
        g = torch.Generator().manual_seed(40 + cmid)
        x = put(_randn(g, 2 * groups, 5, 17, 21), requires_grad=True)
        w1, b1 = put(_randn(g, cmid, 5, 3, 3) * 0.2, requires_grad=True), put(_randn(g, cmid) * 0.1, requires_grad=True)
        w2, b2 = put(_randn(g, cmid, cmid, 3, 3) * 0.2, requires_grad=True), put(_randn(g, cmid) * 0.1, requires_grad=True)
        y = ops.dann_down(x, w1, b1, w2, b2, groups)
        y.backward(put(_randn(g, *y.shape)))
        return dict(y=y, dx=x.grad, dw1=w1.grad, db1=b1.grad, dw2=w2.grad, db2=b2.grad)
    hold(device, down, workspace=True, family="dann_down")


@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
def test_dann_tail(training, device):
    from mcdseg import ops

    def tail(put):
        g = torch.Generator().manual_seed(50)
        h = put(_randn(g, 6, 70), requires_grad=True)
        ps = [put(t, requires_grad=True) for t in (_randn(g, 10, 70) * 0.1, _randn(g, 10) * 0.1, 1 + 0.2 * _randn(g, 10), 0.1 * _randn(g, 10),
                                                    _randn(g, 2, 10) * 0.3, _randn(g, 2) * 0.1)]
        labels = put(torch.tensor([0, 1], dtype=torch.int32))
        rm, rv = put(0.1 * _randn(g, 10)), put(1 + 0.1 * torch.rand(10, generator=g))
        loss, logits = ops.dann_tail(h, *ps, labels, rm, rv, training=training)
        loss.backward(put(torch.tensor([1.0, 0.5])))
        out = dict(loss=loss, logits=logits, dh=h.grad, running_mean=rm, running_var=rv)
        for i, p in enumerate(ps):
            out["grad%d" % i] = p.grad
        return out
    hold(device, tail, workspace=True, family="dann_tail")


# ---------------------------------------------------------------------------------------------------- fusion, multitask
@pytest.mark.parametrize("shape", [(1, 1, 3, 1), (2, 3, 1, 9), (1, 1, 129, 128)], ids=lambda s: "x".join(map(str, s)))
def test_bilinear8(shape, device):
    from mcdseg import ops

    def bilinear(put):
        g = torch.Generator().manual_seed(9)
        x = put(_randn(g, *shape), requires_grad=True)
        y = ops.bilinear8(x)
        y.backward(put(_randn(g, *y.shape)))
        return dict(y=y, dx=x.grad)
    hold(device, bilinear, family="bilinear8")


@pytest.mark.parametrize("grad", [True, False], ids=["grad", "loss-only"])
@pytest.mark.parametrize("n", [1, 5, 1001, 4099])
def test_mse(n, grad, device):
    from mcdseg import ops

    def mse(put):
        g = torch.Generator().manual_seed(n)
        pred, target = put(_randn(g, n), requires_grad=grad), put(_randn(g, n))
        loss = ops.mse_loss(pred, target)
        out = dict(loss=loss)
        if grad:
            loss.backward()
            out["dpred"] = pred.grad
        return out
    hold(device, mse, workspace=True, family="mse")


def test_gate_mix_softmax_and_prob_nll(device):
    """at the smallest shapes of test_fusion_kernels_gpu.py: one element, a ragged float4, both sides of the softmax's class-count
    instantiations, one pixel per image"""
    from mcdseg import ops

    def fusion(put):
        g = torch.Generator().manual_seed(70)
        out = {}
        for shape in ((1,), (3,), (5,), (1, 41, 3, 5)):
            x1, x2, gate = (put(_randn(g, *shape), requires_grad=True) for _ in range(3))
            y = ops.gate_mix(x1, x2, gate)
            y.backward(put(_randn(g, *shape)))
            out.update({"mix%s" % (shape,): y, "dx1%s" % (shape,): x1.grad, "dx2%s" % (shape,): x2.grad, "dgate%s" % (shape,): gate.grad})
        for shape in ((1, 1, 1, 1), (2, 25, 3, 5), (1, 49, 2, 3), (2, 2, 1, 1), (3, 5, 7, 9)):
            n, c, h, w = shape
            z = put(2 * _randn(g, *shape), requires_grad=True)
            p = ops.softmax_channels(z)
            lab = torch.randint(0, c, (n, h, w), generator=g)
            lab[0, 0, 0] = -100 if h * w > 1 else lab[0, 0, 0]
            loss = ops.prob_cross_entropy2d(p, put(lab), put(0.5 + torch.rand(c, generator=g)))
            total = ops.prob_cross_entropy2d(p, put(lab), None, size_average=False)
            (loss + 0.5 * total).backward()
            out.update({"softmax%s" % (shape,): p, "nll%s" % (shape,): loss, "nll_sum%s" % (shape,): total, "dz%s" % (shape,): z.grad})
        return out
    hold(device, fusion, workspace=True, family="gate_mix/softmax/prob_nll")


# ---------------------------------------------------------------------------------------------------- input pipeline, evaluation, utilities
def test_normalize_resize_relabel(device):
    from mcdseg import ops

    def pipeline(put):
        g = torch.Generator().manual_seed(80)
        rgb, one = put(torch.randint(0, 256, (3, 21, 35, 3), generator=g, dtype=torch.uint8)), put(torch.randint(0, 256, (3, 21, 35, 1), generator=g, dtype=torch.uint8))
        dst = put(torch.zeros(3, 4, 21, 35))
        ops.normalize_u8_(dst, rgb, put(torch.tensor([0.4, 0.5, 0.6])), put(torch.tensor([0.2, 0.25, 0.3])), 0)
        ops.normalize_u8_(dst, one, put(torch.tensor([0.3])), put(torch.tensor([0.5])), 3)
        img = put(torch.randint(0, 256, (2, 37, 53, 3), generator=g, dtype=torch.uint8))
        lab = put(torch.randint(0, 41, (2, 37, 53), generator=g, dtype=torch.uint8))
        small = put(torch.randint(0, 256, (1, 9, 7, 3), generator=g, dtype=torch.uint8))
        return dict(normalized=dst, bilinear=ops.resize_u8(img, (32, 24)), nearest=ops.resize_u8(lab, (32, 24), nearest=True),
                    enlarged=ops.resize_u8(small, (20, 31)), enlarged_nearest=ops.resize_u8(small[..., 0].contiguous(), (20, 31), nearest=True),
                    same_width=ops.resize_u8(img, (53, 20)), same_height=ops.resize_u8(img, (30, 37)), relabel=ops.relabel_u8(lab, 0, 255))
    hold(device, pipeline, workspace=True, family="input pipeline")


@pytest.mark.parametrize("n", [1, 64, 65])
def test_confusion_hist(n, device):
    from mcdseg import ops

    def hist(put):
        g = torch.Generator().manual_seed(n)
        gt, pred = put(torch.randint(0, n + 2, (4097,), generator=g)), put(torch.randint(-1, n + 1, (4097,), generator=g))
        h = put(torch.randint(0, 5, (n, n), generator=g))
        ops.confusion_hist_(h, gt, pred)
        ops.confusion_hist_(h, gt, pred)
        return dict(hist=h)
    hold(device, hist, family="confusion_hist")


@pytest.mark.parametrize("math", ["f16x3", "bf16x6"])
def test_split_companions_and_bf16_units(math, device, monkeypatch):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", math)

    def split(put):
        g = torch.Generator().manual_seed(90)
        x, x6 = put(_randn(g, 2, 24, 5, 7)), put(_randn(g, 2, 6, 5, 7))
        cb, bound = ops.split_companion(x)
        cbp, boundp = ops.split_companion_padded(x6, None if ops._scaled() else ops.absmax(x6))
        full = torch.empty(2, 8, 5, 7, device=device)
        ops.check(ops.lib().mcdseg_unsplit_cb(ops._p(cbp), ops._p(boundp), ops.MATH_ID[math], 2, 8, 35, ops._p(full), ops._stream()), "unsplit_cb")
        g21 = put(_randn(g, 1, 24, 3, 7))          # 504 elements: 63 units of 8, a count not divisible by 8 units
        units = ops.pack_bf16_units(g21)
        return dict(unsplit=ops.materialize(x, cb, bound), padded=full[:, :6].contiguous(), padding=full[:, 6:].contiguous(), units=ops.unpack_bf16_units(units))
    hold(device, split, family="split/pack")


@pytest.mark.parametrize("shape", [(2, 64, 6, 8), (2, 24, 5, 7), (1, 41, 3, 5)], ids=lambda s: "x".join(map(str, s)))
def test_stage_join(shape, device, monkeypatch):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")

    def join(put):
        g = torch.Generator().manual_seed(91)
        a, b = put(_randn(g, *shape), requires_grad=True), put(_randn(g, *shape), requires_grad=True)
        y = ops.stage_join(a, b)
        cb, bound = ops._cb_of(y)
        out = dict(y=y)
        if cb is not None:
            out["unsplit"] = ops.materialize(y, cb, bound)
        if bound is not None:
            out["bound"] = bound
        return out
    hold(device, join, family="stage_join")


@pytest.mark.parametrize("off", [0, 3])
@pytest.mark.parametrize("n", [1, 5, 1027, 4099])
def test_absmax(n, off, device):
    from mcdseg import ops

    def absmax(put):
        base = put(_randn(torch.Generator().manual_seed(n + off), n + off))
        return dict(bound=ops.absmax(base[off:]))
    hold(device, absmax, family="absmax")


# ---------------------------------------------------------------------------------------------------- large forward / data-gradient tiles
def _tile_workload(device, cin, cout, k, stride, dil, n, h, w, seed, dgrad=True, addend=True):
    """forward with the fused BatchNorm partial rows and data gradient (alone and with an addend) from pre-split operands; the partial
    rows are compared through ``part[:rows, :, :C]``, not through their channel padding"""
    from mcdseg import ops
    from test_kernels_gpu import _conv_inputs

    def tiles(put):
        x, wt, _, s, pad, d = _conv_inputs((cin, cout, k, stride, dil, h, w, n, False), seed)
        desc = ops.conv_desc(x.shape, wt.shape, stride, pad, d)
        pk = ops.PackedWeights()
        wf, wd, mpf = pk.get(put(wt), desc)
        xg = put(x)
        gyg = put(torch.randn(n, cout, desc.Ho, desc.Wo, generator=torch.Generator().manual_seed(seed + 1)))
        x_cb, x_bound = ops.split_companion(xg)
        gy_cb, gy_bound = ops.split_companion(gyg)
        with named() as names:
            y, part, rows = ops._conv_fprop(desc, xg, wf, None, True, mpf, x_cb, x_bound, pk.w_bound)
            out = dict(y=y, part=part.view(-1)[:rows * 3 * mpf].view(rows, 3, mpf)[:, :, :cout].contiguous())
            if dgrad:
                out["dx"] = ops._conv_dgrad(desc, None, wd, gy_cb, gy_bound, pk.w_bound)
                if addend:
                    other = put(torch.randn(x.shape, generator=torch.Generator().manual_seed(seed + 2)))
                    out["dx_addend"] = ops._conv_dgrad(desc, None, wd, gy_cb, gy_bound, pk.w_bound, addend=other)
        tiles.names = list(names)
        return out
    return tiles


@pytest.mark.parametrize("mode", [3, 2, 4])
@pytest.mark.parametrize("cin,cout", [(64, 512), (512, 64)])
def test_pingpong_tiles(cin, cout, mode, device, monkeypatch, libopt):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    libopt(PP_MIN_ROUNDS=1, PP_WIDE_FILL=101, PINGPONG=mode)
    work = _tile_workload(device, cin, cout, 3, 1, 2, 2, 160, 131, 41)
    hold(device, work, family="ping-pong tiles")
    assert any("conv_gemm_split_pp_kernel" in nm for nm in work.names), work.names
    if mode == 4:
        assert ops.pingpong_kernel_name(cin == 512, wide=True) in work.names, work.names
    if mode == 2:
        assert ops.pingpong_kernel_name(cin == 512, small=True) in work.names, work.names


@pytest.mark.parametrize("case", [(128, 256, 3, 2, 2, 33, 40), (136, 200, 1, 1, 3, 29, 31)], ids=lambda c: "x".join(map(str, c)))
def test_wide_tiles(case, device, monkeypatch, libopt):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    libopt(WIDETILE_MIN_SLOTS=1)
    cin, cout, k, d, n, h, w = case
    work = _tile_workload(device, cin, cout, k, 1, d, n, h, w, 33, addend=False)
    hold(device, work, family="wide tiles")
    assert len(work.names) == 2 and all("4, 2, 1, 4" in nm for nm in work.names), work.names


@pytest.mark.parametrize("form", [0, 1, 2])
def test_stride2_parity_data_gradient(form, device, monkeypatch, libopt):
    from mcdseg import ops
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")
    libopt(DGRAD_INTERLEAVE=form)
    hold(device, _tile_workload(device, 64, 128, 3, 2, 1, 3, 13, 19, 21), family="stride-2 data gradient")


# ---------------------------------------------------------------------------------------------------- weight-gradient variants
# (Cin, Cout, k, stride, dil, H, W, N), arithmetic, library options, mcdseg_conv_wgrad_variant, the kernel named
WGRAD_VARIANTS = [
    ((136, 200, 3, 1, 2, 13, 19, 2), "f16x3", {}, 12, "conv_wgrad_split_tr_kernel<SplitF16x3, 2, 2, 3>"),     # transposed read, 128 rows
    ((72, 80, 3, 1, 1, 8, 8, 3), "f16x3", {}, 12, "conv_wgrad_split_tr_kernel<SplitF16x3, 2, 2, 3>"),        # 72 x 80: above 64 on both sides, still 128 rows
    ((48, 64, 3, 1, 2, 13, 19, 2), "f16x3", {}, 14, "conv_wgrad_split_tr64_kernel<SplitF16x3>"),             # the 64-row kernel, ragged channel groups
    ((6, 16, 7, 1, 1, 21, 45, 2), "f16x3", {}, 15, None),                                                    # thin transposed read, padded companion
    ((16, 16, 3, 1, 1, 21, 45, 2), "f16x3", {}, 15, None),
    ((392, 504, 3, 1, 4, 29, 37, 8), "f16x3", dict(WGRAD_PP=2), 17, "conv_wgrad_split_pp_kernel<SplitF16x3>"),  # the slab plan
    ((392, 504, 3, 1, 4, 29, 37, 8), "f16x3", dict(WGRAD_PP=1), 17, "conv_wgrad_split_pp_kernel<SplitF16x3>"),  # stream-K
    ((96, 128, 3, 1, 1, 45, 50, 16), "f16x3", dict(WGRAD_PP3=1), 18, "conv_wgrad_split_pp3_kernel<SplitF16x3>"),  # a row of taps
    ((264, 512, 3, 1, 4, 29, 37, 6), "f16x3", dict(WGRAD_BIG=1, WGRAD_PP=0), 13, "conv_wgrad_split_tr_kernel<SplitF16x3, 4, 2, 3>"),  # the large tile
]


@pytest.mark.parametrize("case,math,options,variant,kernel", WGRAD_VARIANTS, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else None)
def test_wgrad_variants_with_presplit_operands(case, math, options, variant, kernel, device, monkeypatch, libopt):
    from mcdseg import ops
    from test_kernels_gpu import _conv_inputs
    monkeypatch.setattr(ops, "CONV_MATH", math)
    libopt(**options)
    cin, cout, k, s, d, h, w, n = case
    x, wt, _, s, pad, d = _conv_inputs((cin, cout, k, s, d, h, w, n, False), 43)
    desc = ops.conv_desc(x.shape, wt.shape, s, pad, d)
    assert ops.lib().mcdseg_conv_wgrad_variant(ctypes.byref(desc), ops.MATH_ID[math], 1) == variant
    gy = torch.randn(n, cout, desc.Ho, desc.Wo, generator=torch.Generator().manual_seed(44))
    seen = []

    def wgrad(put):
        xg, gyg = put(x), put(gy)
        x_cb, x_bound = ops.split_companion(xg) if cin % 8 == 0 else ops.split_companion_padded(xg)
        gy_cb, gy_bound = ops.split_companion(gyg)
        assert x_cb is not None and gy_cb is not None
        with named() as names:
            dw = ops._conv_wgrad(desc, xg, gyg, x_cb, gy_cb, x_bound, gy_bound)
        seen.append(list(names))
        return dict(dw=dw)
    hold(device, wgrad, workspace=True, family="wgrad variant %d" % variant)
    if kernel is not None:
        assert all(names == [kernel] for names in seen), seen


def test_conv_cases_from_fp32_operands(device):
    """the three passes of every geometry of ``CONV_CASES`` from fp32 operands (no companion): what test_conv_fprop_dgrad_wgrad runs"""
    from mcdseg import ops
    from test_kernels_gpu import CONV_CASES, _conv_inputs

    def passes(put):
        out = {}
        for i, case in enumerate(CONV_CASES):
            x, wt, b, s, pad, d = _conv_inputs(case, 7)
            desc = ops.conv_desc(x.shape, wt.shape, s, pad, d)
            packed = ops.PackedWeights()
            xg = put(x)
            wf, wd, mpf = packed.get(put(wt), desc)
            y, _, _ = ops._conv_fprop(desc, xg, wf, put(b) if b is not None else None, False, mpf, w_bound=packed.w_bound)
            gy = put(torch.randn(y.shape, generator=torch.Generator().manual_seed(8)))
            out.update({"y%d" % i: y, "dx%d" % i: ops._conv_dgrad(desc, gy, wd, w_bound=packed.w_bound), "dw%d" % i: ops._conv_wgrad(desc, xg, gy)})
        return out
    hold(device, passes, workspace=True, family="CONV_CASES, fp32 operands")


# ---------------------------------------------------------------------------------------------------- uncertain loss
@pytest.mark.parametrize("c,t", [(20, 4), (48, 1)])
def test_uncertain_loss(c, t, device):
    from mcdseg import ops

    def uncertain(put):
        g = torch.Generator().manual_seed(60 + c)
        n, hi, wi = 2, 3, 5
        s = put(_randn(g, n, c, hi, wi), requires_grad=True)
        w_up, w_std = put(_randn(g, c, 1, 16, 16) * 0.2, requires_grad=True), put(_randn(g, c, 1, 16, 16) * 0.2, requires_grad=True)
        lab = torch.randint(0, c, (n, 8 * hi, 8 * wi), generator=g)
        lab[0, 1, :6] = -100
        keep = (torch.rand(t, n, c, generator=g) >= 0.2).to(torch.uint8)
        base, unc = ops.up8_uncertain_loss(s, w_up, w_std, put(lab), put(0.5 + torch.rand(c, generator=g)), put(keep), put(torch.rand(t, generator=g)))
        (base * 0.7 + (unc * put(torch.tensor([1.0, 0.5]))).sum()).backward()
        return dict(base=base, uncertain=unc, ds=s.grad, dw_up=w_up.grad, dw_std=w_std.grad, std_sum=ops.up8_std_sum(s.detach(), w_std.detach(), c - 1))
    hold(device, uncertain, workspace=True, family="uncertain loss")


# ---------------------------------------------------------------------------------------------------- boundary branch
@pytest.mark.parametrize("shape", [(2, 8, 16), (2, 5, 13), (1, 1, 1)], ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("dtype", [torch.int64, torch.uint8], ids=["int64", "uint8"])
def test_label_boundary(dtype, shape, device):
    from mcdseg import ops

    def boundary(put):
        lab = torch.randint(0, 5, shape, generator=torch.Generator().manual_seed(3)).to(dtype)
        return dict(boundary=ops.label_boundary(put(lab)))
    hold(device, boundary, family="label_boundary")


@pytest.mark.parametrize("h8,w8", [(1, 1), (2, 3)])
def test_boundary_head_and_its_losses(h8, w8, device):
    from mcdseg import ops

    def head(put):
        g = torch.Generator().manual_seed(71)
        n, h, w = 2, 8 * h8, 8 * w8
        maps = lambda: [put(_randn(g, n, 1, 4 * h8, 4 * w8), requires_grad=True), put(_randn(g, n, 1, 2 * h8, 2 * w8), requires_grad=True),
                        put(_randn(g, n, 1, h8, w8), requires_grad=True)]
        out = {}
        s = maps()
        p = ops.boundary_head(*s)
        p.backward(put(_randn(g, n, 1, h, w)))
        out.update(p=p, d1=s[0].grad, d2=s[1].grad, d3=s[2].grad)
        labels = put(torch.randint(0, 4, (n, h, w), generator=g))
        s = maps()
        loss = ops.boundary_head_bce(*s, labels)
        loss.backward()
        out.update(fused=loss, f1=s[0].grad, f2=s[1].grad, f3=s[2].grad)
        wide = put((torch.rand(n, 3, h, w, generator=g) > 0.7).float())
        for tag, target in (("fp32", put(torch.rand(n, 1, h, w, generator=g))), ("uint8", put((torch.rand(n, h, w, generator=g) > 0.7).to(torch.uint8))),
                            ("slice", wide[:, 1:2])):
            s = maps()
            loss = ops.boundary_head_bce_target(*s, target)
            loss.backward()
            out.update({tag: loss, tag + "/d1": s[0].grad, tag + "/d2": s[1].grad, tag + "/d3": s[2].grad})
        return out
    hold(device, head, workspace=True, family="boundary head")


@pytest.mark.parametrize("shape", [(1, 3, 7), (2, 8, 16)], ids=lambda s: "x".join(map(str, s)))
def test_bce2d(shape, device):
    from mcdseg import ops

    def bce(put):
        g = torch.Generator().manual_seed(72)
        out = {}
        for tag, target in (("fp32", torch.rand(*shape, generator=g)), ("uint8", (torch.rand(*shape, generator=g) > 0.6).to(torch.uint8))):
            p = put(torch.rand(*shape, generator=g) * 0.98 + 0.01, requires_grad=True)
            loss, beta = ops.bce2d(p, put(target), return_beta=True)
            loss.backward()
            out.update({tag: loss, tag + "/beta": beta, tag + "/dp": p.grad})
        return out
    hold(device, bce, workspace=True, family="bce2d")


@pytest.mark.parametrize("heads", [1, 2])
def test_seg2bd(heads, device):
    from mcdseg import ops

    def seg2bd(put):
        g = torch.Generator().manual_seed(73)
        n, c, hi, wi = 2, 5, 3, 4
        z1 = put(_randn(g, n, c, hi, wi), requires_grad=True)
        z2 = put(_randn(g, n, c, hi, wi), requires_grad=True) if heads == 2 else None
        wt, b = put(_randn(g, 1, c, 5, 5) * 0.2, requires_grad=True), put(_randn(g, 1) * 0.1, requires_grad=True)
        target = put((torch.rand(n, 1, 8 * hi, 8 * wi, generator=g) > 0.7).to(torch.uint8))
        l1, l2, beta = ops.seg2bd_bce(z1, z2, wt, b, target, return_beta=True)
        (l1 if l2 is None else l1 + 0.5 * l2).backward()
        out = dict(loss1=l1, beta=beta, dz1=z1.grad, dw=wt.grad, db=b.grad)
        if heads == 2:
            out.update(loss2=l2, dz2=z2.grad)
        return out
    hold(device, seg2bd, workspace=True, family="seg2bd")


# ---------------------------------------------------------------------------------------------------- joint augmentation, refinement
def test_joint_augment_entry_points(device, golden):
    """the four entry points at the smallest golden shape (``joint_ref.SHAPES[0]``: 17 x 23 cropped to 11 x 13, an odd width), on the
    golden images: three samples that differ in flip, rotation mode and crop corner in one launch"""
    import joint_ref as J
    from mcdseg import augment, ops
    fx = golden.npz("joint_augment_small.npz")
    h, w = J.SHAPES[0]
    tw, th = J.CROP_WH[(h, w)]

    def joint(put):
        rows = [augment.sample_params(f, a, x1, y1, w, h) for f, a, x1, y1 in ((True, 7.3, 0, 0), (False, 90.0, w - tw, h - th), (False, -10.0, 5, 3))]
        params = augment.JointParams([r[0] for r in rows], [r[1] for r in rows], (h, w), (th, tw))
        tables = (put(torch.from_numpy(params.affine)), put(torch.from_numpy(params.geom)))
        rgb = put(torch.from_numpy(fx["img_s0"][..., :3].copy())[None].expand(3, h, w, 3).contiguous())
        lbl = put(torch.from_numpy(fx["lbl_s0"].copy())[None].expand(3, h, w).contiguous())
        dst = put(torch.zeros(3, 4, th, tw))
        ops.joint_augment_normalize_u8_(dst, rgb, tables, put(torch.tensor([0.4, 0.5, 0.6])), put(torch.tensor([0.2, 0.25, 0.3])), c_off=1)
        return dict(image=ops.joint_augment_u8(rgb, tables, (th, tw)), label=ops.joint_augment_u8(lbl, tables, (th, tw), nearest=True), normalized=dst,
                    relabel=ops.joint_augment_relabel_u8(lbl, tables, (th, tw), 255, 40))
    hold(device, joint, family="joint augment")


@pytest.mark.parametrize("hw", [(1, 1), (1, 97), (33, 65)], ids=lambda s: "x".join(map(str, s)))
def test_refine_regions_and_vote(hw, device):
    import numpy as np
    import refine_ref as R
    from mcdseg import ops

    def refine(put):
        h, w = hw
        bd = np.stack([R.bernoulli(h, w, 0.3, 5), R.bernoulli(h, w, 0.6, 8)])
        seg = np.stack([R.seeded_seg(h, w, 6), R.seeded_seg(h, w, 7)])
        bd, seg = put(torch.from_numpy(bd)), put(torch.from_numpy(seg))
        regions = ops.boundary_regions(bd, R.THRE)
        return dict(regions=regions, refined=ops.refine_labels(seg, regions, 2, 500), one_call=ops.refine_labels_by_boundary(seg, bd, R.THRE, 0, 79333))
    hold(device, refine, workspace=True, family="refine")


# ---------------------------------------------------------------------------------------------------- optimisers
@pytest.mark.parametrize("opt", ["sgd", "adam"])
def test_flat_optimisers(opt, device, monkeypatch):
    """two steps of the flat optimisers; the flat buffers come from the patched ``torch.zeros``.  The first parameter is a stem's weight
    whose packed image (with its weight bound) is rebuilt after each step and read by a forward pass"""
    from mcdseg import ops, optim
    from models.drn import Conv2d
    monkeypatch.setattr(ops, "CONV_MATH", "f16x3")

    def steps(put):
        g = torch.Generator().manual_seed(95)
        conv = Conv2d(6, 16, 7, padding=3, bias=False)
        with torch.no_grad():
            conv.weight.copy_(_randn(g, 16, 6, 7, 7) * 0.05)
        place(conv, put)
        params = [conv.weight] + [torch.nn.Parameter(put(_randn(g, *s))) for s in ((16,), (33, 5, 3, 3), (7,))]
        o = optim.FlatSGD(params, lr=0.1, momentum=0.9, weight_decay=1e-4) if opt == "sgd" else optim.FlatAdam(params, lr=1e-2, weight_decay=1e-4)
        x = put(_randn(g, 2, 6, 9, 13))
        out = {}
        for step in range(2):
            for p in params:
                p.grad = put(_randn(g, *p.shape))
            o.step()
            desc = ops.conv_desc(x.shape, conv.weight.shape, 1, 3, 1)
            wf, wd, mpf = conv._packed.get(conv.weight, desc)
            out["y%d" % step], _, _ = ops._conv_fprop(desc, x, wf, None, False, mpf, w_bound=conv._packed.w_bound)
        for i, p in enumerate(params):
            out["p%d" % i] = p.data
        for i, f in enumerate(o.flat_buffers()):
            out["flat%d" % i] = f
        return out
    hold(device, steps, family="flat %s" % opt)


# ---------------------------------------------------------------------------------------------------- one whole step
@pytest.mark.parametrize("dtype", ["f16x3", "f16"])
def test_whole_mcd_step(dtype, device, golden, monkeypatch):
    """``MCDSolver.step`` on the small models of test_model_gpu.py's drop-in-loop test, at that test's batch, with the side-stream weight
    gradients at their default: the step's losses and a checksum of every parameter and buffer"""
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from loss import CrossEntropyLoss2d, get_prob_distance_criterion
    from mcdseg import ops
    from models.model_util import get_models, get_optimizer
    from recipe import fill_state_, make_batch
    from solvers.solver import MCDSolver
    monkeypatch.setattr(ops, "CONV_MATH", "f16x1" if dtype == "f16" else "f16x3")
    monkeypatch.setattr(ops, "ACT_STORAGE", "compact" if dtype == "f16" else "fp32")
    assert ops.OVERLAP_WGRAD == "2"
    tr = golden.json("traces.json")["mcd_small"]
    n, ch, h, w = tr["shape"]

    def step(put):
        models = get_models("drn_d_38", 6, 41)
        for m, seed in zip(models, (11, 12, 13)):
            fill_state_(m, seed)
            place(m, put).train()
        g, f1, f2 = models
        s, l, t = (put(v) for v in make_batch(tr["seed_batch"], n, ch, h, w, 41))
        og = get_optimizer(g.parameters(), "sgd", 1e-3, 0.9, 2e-5)
        of = get_optimizer(list(f1.parameters()) + list(f2.parameters()), "sgd", 1e-3, 0.9, 2e-5)
        cw = torch.ones(41)
        cw[40] = 0
        before = ops.WGRAD_STREAM_STATS["deferred"]
        solver = MCDSolver(g, f1, f2, og, of, CrossEntropyLoss2d(put(cw)), get_prob_distance_criterion("diff"), num_k=4)
        c_loss, d_loss = solver.step(s, l, t)
        assert ops.WGRAD_STREAM_STATS["deferred"] > before, "no weight gradient ran on the side stream"
        out = dict(c_loss=torch.as_tensor(c_loss).detach().reshape(1), d_loss=torch.as_tensor(d_loss).detach().reshape(1))
        for i, m in enumerate(models):
            for k, v in m.state_dict().items():
                out["%d.%s" % (i, k)] = v
        return out
    hold(device, step, workspace=True, family="MCDSolver.step %s" % dtype)
