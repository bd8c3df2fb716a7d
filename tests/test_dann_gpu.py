"""GPU: the fused domain classifier of the DANN baseline (csrc/dann.hip through the C ABI), DRNSegDomainClassifier, and dann_trainer.py
end to end, against tests/golden/dann_small.npz (the real reference in fp64).

The tolerance rule is the project's (tests/truth.py, uncertain_ref.rel_to_max): per output tensor, the kernel's distance to the fp64
truth relative to the truth's largest magnitude, in units of the distance of the reference's OWN fp32 run (the golden "f32/" arrays)
to the same truth.  MARGIN = 4: the kernel and torch's fp32 operators round the same products and differ in the order they sum them,
so the two distances are two draws of one distribution; over the dozens of short sums a tensor's maximum is taken from, one draw
exceeds another by a factor of 2 to 3 now and then, and 4 leaves that room and no more -- a ratio in the tens is a bug.  Where the
reference's fp32 run is exact or nearly so (the identity-kernel tie cases; a bias gradient of a few terms) the floor is 4 fp32 ulps of
the tensor's largest magnitude.  The bound is never taken from the kernel's output; each figure is printed before it is asserted.
The tail kernels carry the BatchNorm1d arithmetic in fp64 (csrc/dann.hip says why), so on the ill-conditioned n = 2 case they sit far
below the fp32 reference's distance, not near it.  Measured ratios: DESIGN.md section 4.9.
"""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import dann_ref as R
from dann_ref import DOWN, TAIL, case

pytestmark = pytest.mark.gpu

MARGIN = 4.0
FLOOR = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def fx(golden):
    return golden.npz("dann_small.npz")


def hold(fx, name, got, scales=None):
    """every tensor of ``got`` within max(MARGIN units, FLOOR) of the golden fp64; returns {key: (error, unit)}"""
    out, bad = {}, []
    for k, v in got.items():
        truth, f32 = fx["%s/f64/%s" % (name, k)], fx["%s/f32/%s" % (name, k)]
        scale = (scales or {}).get(k)
        err, unit = R.rel_to_max(v, truth, scale), R.rel_to_max(f32, truth, scale)
        print("%-14s %-13s error %.3e   the reference's fp32 %.3e   ratio %s   bound %.3e"
              % (name, k, err, unit, "%.2f" % (err / unit) if unit > 0 else "-", max(MARGIN * unit, FLOOR)))
        out[k] = (err, unit)
        if err > max(MARGIN * unit, FLOOR):
            bad.append((k, err, unit))
    assert not bad, (name, bad)
    return out


def _t(a, dev, dtype=torch.float32):
    return torch.as_tensor(np.asarray(a)).to(dtype).to(dev).contiguous()


def _p(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def down_abi(d, dev, groups=1, want_dx=True):
    """mcdseg_dann_down_fwd / _bwd through ctypes"""
    import mcdseg
    L = mcdseg.lib()
    x, w1, b1, w2, b2, dy = (_t(d[k], dev) for k in ("x", "w1", "b1", "w2", "b2", "dy"))
    n, cin, h, w = x.shape
    cm = w1.shape[0]
    y = torch.full((n, cm, h // 2, w // 2), float("nan"), device=dev)
    assert L.mcdseg_dann_down_fwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), n, cin, cm, h, w, _stream()) == 0, L.mcdseg_last_error()
    dx = torch.full_like(x, float("nan")) if want_dx else None
    dw1, db1, dw2, db2 = (torch.full_like(t, float("nan")) for t in (w1, b1, w2, b2))
    nbytes = L.mcdseg_dann_down_workspace_bytes(n, cin, cm, h, w)
    ws = torch.empty(nbytes // 4 + 1, device=dev)
    rc = L.mcdseg_dann_down_bwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(dy), _p(dx), _p(dw1), _p(db1), _p(dw2), _p(db2), n, cin, cm, h, w,
                                groups, _p(ws), ctypes.c_size_t(nbytes), _stream())
    assert rc == 0, L.mcdseg_last_error()
    torch.cuda.synchronize()
    out = {"y": y, "dw1": dw1, "db1": db1, "dw2": dw2, "db2": db2}
    if want_dx:
        out["dx"] = dx
    return {k: v.cpu().numpy() for k, v in out.items()}


def tail_abi(d, dev, want_dh=True):
    """mcdseg_dann_tail_fwd / _bwd through ctypes"""
    import mcdseg
    L = mcdseg.lib()
    h, w1, b1, gamma, beta, rm, rv, w2, b2, up = (_t(d[k], dev) for k in ("h", "w1", "b1", "gamma", "beta", "rm", "rv", "w2", "b2", "up"))
    labels = _t(d["labels"], dev, torch.int32)
    groups, training = int(d["groups"]), int(d["training"])
    rows, f = h.shape
    n = rows // groups
    loss, logits = torch.full((groups,), float("nan"), device=dev), torch.full((rows, 2), float("nan"), device=dev)
    save = torch.empty(L.mcdseg_dann_tail_save_bytes(groups, n) // 8 + 1, dtype=torch.float64, device=dev)
    rc = L.mcdseg_dann_tail_fwd(_p(h), _p(labels), _p(w1), _p(b1), _p(gamma), _p(beta), _p(rm), _p(rv), _p(w2), _p(b2), 0.1, 1e-5, training,
                                _p(loss), _p(logits), _p(save), groups, n, f, _stream())
    assert rc == 0, L.mcdseg_last_error()
    dh = torch.full_like(h, float("nan")) if want_dh else None
    g = {k: torch.full(s, float("nan"), device=dev) for k, s in (("dw1", (10, f)), ("db1", (10,)), ("dgamma", (10,)), ("dbeta", (10,)),
                                                               ("dw2", (2, 10)), ("db2", (2,)))}
    nbytes = L.mcdseg_dann_tail_workspace_bytes(groups, n)
    ws = torch.empty(nbytes // 4 + 1, device=dev)
    rc = L.mcdseg_dann_tail_bwd(_p(h), _p(labels), _p(w1), _p(gamma), _p(beta), _p(w2), _p(logits), _p(save), _p(up), _p(dh), _p(g["dw1"]),
                                _p(g["db1"]), _p(g["dgamma"]), _p(g["dbeta"]), _p(g["dw2"]), _p(g["db2"]), training, groups, n, f, _p(ws),
                                ctypes.c_size_t(nbytes), _stream())
    assert rc == 0, L.mcdseg_last_error()
    torch.cuda.synchronize()
    out = dict(g, loss=loss, logits=logits, running_mean=rm, running_var=rv)
    if want_dh:
        out["dh"] = dh
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.mark.parametrize("name", DOWN)
def test_down_kernels_against_the_reference(fx, device, name):
    d = case(fx, name)
    got = down_abi(d, device)
    assert all(np.isfinite(v).all() for v in got.values())
    hold(fx, name, got)
    if "ties" in name:  # the integer facts, exactly: which element of a tied window takes the gradient, nothing for an all-zero window
        for k, v in got.items():
            assert np.array_equal(v, fx["%s/f64/%s" % (name, k)]), k
        dx, dy = got["dx"][0, 0], d["dy"][0, 0]
        assert dx[0, 1] == dy[0, 0] and dx[0, 2] == dy[0, 1] and dx[2, 3] == dy[1, 1] and np.count_nonzero(dx) == 3
        if name.endswith("odd"):  # ... and nothing in the row and the column the pooling drops
            assert not dx[4].any() and not dx[:, 4].any()
    # the input gradient is optional (the trainer's second update): the parameter gradients do not change when it is left out
    if name == "down/b":
        again = down_abi(d, device, want_dx=False)
        assert all(np.array_equal(again[k], got[k]) for k in again)


@pytest.mark.parametrize("name", TAIL)
def test_tail_kernels_against_the_reference(fx, device, name):
    d = case(fx, name)
    got = tail_abi(d, device)
    assert all(np.isfinite(v).all() for v in got.values())
    hold(fx, name, got, scales={"db1": float(d["db1_scale"])} if int(d["training"]) else None)
    if not int(d["training"]):  # --fix_bn: the running statistics normalise and are left alone, bit for bit
        assert np.array_equal(got["running_mean"], d["rm"]) and np.array_equal(got["running_var"], d["rv"])


def test_backward_is_bit_reproducible(fx, device):
    a, b = (down_abi(case(fx, "down/b"), device) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)
    a, b = (tail_abi(case(fx, "tail/b"), device) for _ in range(2))
    assert all(np.array_equal(a[k], b[k]) for k in a)


def test_refused_shapes_launch_nothing(fx, device):
    import mcdseg
    L = mcdseg.lib()
    # one row per group in training mode: torch refuses it, and so does the entry point
    d = case(fx, "tail/a")
    h, w1, b1, gamma, beta, rm, rv, w2, b2 = (_t(d[k], device) for k in ("h", "w1", "b1", "gamma", "beta", "rm", "rv", "w2", "b2"))
    labels = torch.zeros(4, dtype=torch.int32, device=device)
    loss, logits = torch.full((4,), 7.0, device=device), torch.full((4, 2), 7.0, device=device)
    save = torch.zeros(256, dtype=torch.float64, device=device)  # (4 groups of 1 row: 160 + 640 bytes)
    args = (_p(h), _p(labels), _p(w1), _p(b1), _p(gamma), _p(beta), _p(rm), _p(rv), _p(w2), _p(b2), 0.1, 1e-5)
    rc = L.mcdseg_dann_tail_fwd(*args, 1, _p(loss), _p(logits), _p(save), 4, 1, 6, _stream())
    assert rc < 0 and b"at least 2 rows" in L.mcdseg_last_error()
    torch.cuda.synchronize()
    assert (loss == 7).all() and (logits == 7).all() and np.array_equal(rm.cpu().numpy(), d["rm"])
    assert L.mcdseg_dann_tail_fwd(*args, 0, _p(loss), _p(logits), _p(save), 4, 1, 6, _stream()) == 0  # (eval mode takes one row)
    # more input channels than the backward's tile holds in LDS
    x = torch.zeros((1, 64, 8, 8), device=device)
    w1, b1, w2, b2 = torch.zeros((10, 64, 3, 3), device=device), torch.zeros(10, device=device), torch.zeros((10, 10, 3, 3), device=device), torch.zeros(10, device=device)
    y = torch.full((1, 10, 4, 4), 7.0, device=device)
    rc = L.mcdseg_dann_down_fwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), 1, 64, 10, 8, 8, _stream())
    assert rc < 0 and b"bytes of LDS" in L.mcdseg_last_error()
    dws = [torch.full_like(t, 7.0) for t in (x, w1, b1, w2, b2)]
    ws = torch.zeros(1 << 16, device=device)
    rc = L.mcdseg_dann_down_bwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), *[_p(t) for t in dws], 1, 64, 10, 8, 8, 1, _p(ws),
                                ctypes.c_size_t(ws.numel() * 4), _stream())
    assert rc < 0 and b"bytes of LDS" in L.mcdseg_last_error()
    rc = L.mcdseg_dann_down_fwd(_p(x), _p(w1), _p(b1), _p(w2), _p(b2), _p(y), 1, 64, 5, 8, 8, _stream())
    assert rc < 0 and b"must be 1 or 10" in L.mcdseg_last_error()
    torch.cuda.synchronize()
    assert (y == 7).all() and all((t == 7).all() for t in dws)


def test_pair_equals_two_calls_beyond_sixteen_tiles_per_domain(device):
    """72 x 88 score maps: 30 tiles per sample, 60 per domain -- the second stage of the parameter gradients walks its strided loop
    several times per domain, as at the trainer's geometry, and the sum over both domains still equals two calls' bit for bit"""
    from models.dilated_fcn import DRNSegDomainClassifier
    g = torch.Generator().manual_seed(5)
    src, tgt = (torch.randn(2, 5, 72, 88, generator=g).to(device) for _ in range(2))
    torch.manual_seed(6)
    start = DRNSegDomainClassifier(5, fc_in=18 * 22).state_dict()
    for k in ("conv1.conv1.bias", "conv1.conv2.bias", "conv2.conv1.bias", "conv2.conv2.bias"):
        start[k] = torch.full_like(start[k], 0.5)  # (the default draw leaves the second DownConv's one channel dead: no gradient to compare)
    runs = []
    for pair in (True, False):
        d = DRNSegDomainClassifier(5, fc_in=18 * 22)
        d.load_state_dict(start)
        d.to(device).train()
        if pair:
            d.forward_pair(src, tgt)[0].sum().backward()
        else:
            (d.domain_loss(src, 1)[0] + d.domain_loss(tgt, 0)[0]).backward()
        torch.cuda.synchronize()
        runs.append({k: p.grad for k, p in d.named_parameters()})
    for k in runs[0]:
        assert torch.isfinite(runs[0][k]).all() and torch.equal(runs[0][k], runs[1][k]), k
    assert float(runs[0]["conv1.conv1.weight"].abs().max()) > 0


def test_score_map_size_is_what_the_trunk_returns(device, monkeypatch):
    """models.dilated_fcn.score_map_hw, which sizes D's fc1, against what the trunk really returns (odd sizes both ways)"""
    monkeypatch.setenv("MCDSEG_PRETRAINED", "0")
    from models.dilated_fcn import DRNSegBase, score_map_hw
    g = DRNSegBase("drn_d_38", 5, pretrained=False, input_ch=3).to(device).train()
    with torch.no_grad():
        out = g(torch.randn(2, 3, 65, 87, device=device))
    assert tuple(out.shape[2:]) == score_map_hw(g.base, 65, 87) == (9, 11)


def _load(m, fx, prefix, dev):
    m.load_state_dict({k[len(prefix):]: torch.as_tensor(fx[k]) for k in fx.files if k.startswith(prefix)})
    return m.to(dev).train()


def test_forward_pair_equals_two_calls_bit_for_bit(fx, device):
    from models.dilated_fcn import DRNSegDomainClassifier
    g = torch.Generator().manual_seed(3)
    src, tgt = (torch.randn(3, 5, 16, 24, generator=g).to(device) for _ in range(2))
    runs = []
    for pair in (True, False):
        d = _load(DRNSegDomainClassifier(5, fc_in=24), fx, "step/init/d.", device)
        a, b = src.clone().requires_grad_(True), tgt.clone().requires_grad_(True)
        if pair:
            loss, logits = d.forward_pair(a, b)
            loss.sum().backward()
        else:
            (l1, g1), (l0, g0) = d.domain_loss(a, 1), d.domain_loss(b, 0)
            (l1 + l0).backward()
            loss, logits = torch.stack([l1, l0]), torch.cat([g1, g0])
        torch.cuda.synchronize()
        runs.append(dict({"loss": loss, "logits": logits, "dsrc": a.grad, "dtgt": b.grad}, **{"grad." + k: p.grad for k, p in d.named_parameters()},
                         **{"buf." + k: v for k, v in d.named_buffers()}))
    for k in runs[0]:
        assert torch.equal(runs[0][k], runs[1][k]), k
    assert int(runs[0]["buf.bn1.num_batches_tracked"]) == 2
    # the reference's signature: one domain's logits through the same kernels
    d = _load(DRNSegDomainClassifier(5, fc_in=24), fx, "step/init/d.", device)
    assert torch.equal(d(src), runs[0]["logits"][:3])
    with torch.no_grad():
        assert not d(src).requires_grad
    with pytest.raises(RuntimeError, match="domain_loss"):  # the reference's criterion_d(model_d(x), lbl).backward(): told where to go
        torch.nn.functional.cross_entropy(d(src), torch.ones(3, dtype=torch.long, device=device)).backward()
    with pytest.raises(ValueError, match="fc_in=24"):
        DRNSegDomainClassifier(5).to(device)(src)


def test_two_iterations_follow_the_reference(fx, device):
    """dann_trainer's two updates over the product's F and D (G: the golden case's 1x1 convolution, a torch module) against the reference's
    fp64 trajectory after each of the four updates, and the carried-over gradient: D's first step is the reference's, which the golden
    data shows to be far from a step on update 2's gradient alone (tests/test_dann_host.py asserts that on the golden numbers)"""
    import dann_trainer
    from loss import CrossEntropyLoss2d
    from models.dilated_fcn import DRNSegDomainClassifier, DRNSegPixelClassifier
    from models.model_util import get_optimizer
    lr, momentum, wd = (float(v) for v in fx["step/hyper"])
    mods = {"g": _load(torch.nn.Conv2d(3, 5, 1), fx, "step/init/g.", device), "f": _load(DRNSegPixelClassifier(5), fx, "step/init/f.", device),
            "d": _load(DRNSegDomainClassifier(5, fc_in=24), fx, "step/init/d.", device)}
    opts = {k: get_optimizer(m.parameters(), "sgd", lr, momentum, wd) for k, m in mods.items()}
    criterion = CrossEntropyLoss2d(_t(fx["step/cw"], device))
    src, tgt, lbl = _t(fx["step/src"], device), _t(fx["step/tgt"], device), _t(fx["step/lbl"], device, torch.int64)

    def check(it, update):
        for name in (("g", "f") if update == 1 else ("d",)):
            got = {k: v.detach().cpu().numpy() for k, v in mods[name].state_dict().items() if v.dtype.is_floating_point}
            # a D tensor is measured against its own magnitude or, where that is smaller (bn1.bias starts at zero and D's step is the
            # difference of two nearly equal gradients), against the size of a plain step on update 2's gradient -- golden numbers both
            scales = {"i%du%d/d.%s" % (it, update, k): max(float(np.abs(fx["step/f64/i%du%d/d.%s" % (it, update, k)]).max()),
                                                        float(np.abs(fx["step/f64/d_alone/d." + k] - fx["step/init/d." + k].astype(np.float64)).max()))
                      for k in got} if name == "d" else None
            hold(fx, "step", {"i%du%d/%s.%s" % (it, update, name, k): v for k, v in got.items()}, scales=scales)
            for k, v in mods[name].state_dict().items():
                if not v.dtype.is_floating_point:
                    assert int(v) == int(fx["step/f64/i%du%d/%s.%s" % (it, update, name, k)]), k

    for it in range(2):
        c = dann_trainer.update_g_f(mods["g"], mods["f"], mods["d"], opts["g"], opts["f"], criterion, src, lbl, tgt)
        check(it, 1)
        # D's gradient of update 1 is left in place for update 2 (fc1.bias may hold exact zeros: behind BatchNorm1d its gradient cancels)
        assert all(p.grad is not None for p in mods["d"].parameters()) and float(mods["d"].fc2.weight.grad.abs().max()) > 0
        dl = dann_trainer.update_d(mods["g"], mods["d"], opts["g"], opts["f"], opts["d"], src, tgt)
        check(it, 2)
        for key, v in (("c_loss", float(c)), ("d_loss", float(dl))):  # the logged scalars, by the same rule
            truth, f32 = float(fx["step/f64/" + key][it]), float(fx["step/f32/" + key][it])
            bound = max(MARGIN * abs(f32 - truth), FLOOR * abs(truth))
            print("step %s[%d] %.8f (fp64 %.8f, the reference's fp32 %.8f): error %.3e, bound %.3e" % (key, it, v, truth, f32, abs(v - truth), bound))
            assert abs(v - truth) <= bound
    # not the other step: on the golden numbers the two differ by far more than the bound just held
    ref, alone = fx["step/f64/i0u2/d.fc2.weight"], fx["step/f64/d_alone/d.fc2.weight"]
    assert R.rel_to_max(alone, ref) > 100 * max(MARGIN * R.rel_to_max(fx["step/f32/i0u2/d.fc2.weight"], ref), FLOOR)


def test_trainer_resume_tester_and_adjust_lr(tmp_path, fx, capsys):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import adapt_tester
    import dann_trainer
    import util
    from PIL import Image
    out = str(tmp_path / "out")
    flags = ["--net", "drn_d_22", "--input_ch", "3", "-b", "2", "--train_img_shape", "96", "64", "--synthetic", "--no_pretrained",
             "--epochs", "1", "--max_iter", "1", "--no_tflog", "--synthetic_len", "8", "--adjust_lr", "--lr", "0.004"]
    assert dann_trainer.main(["suncg", "nyu", "--base_outdir", out] + flags) == 0
    pth = os.path.join(out, "suncg-train2nyu-train_3ch", "pth")
    ck_fn = os.path.join(pth, "DANN-normal-drn_d_22-1.pth.tar")
    ck = util.load_checkpoint(ck_fn)
    # (the reference also writes "res" and "net" beside args, which holds both; no trainer on the common skeleton does: INTEGRATION.md)
    assert sorted(ck) == sorted(["epoch", "args", "g_state_dict", "f1_state_dict", "d_state_dict", "optimizer_g", "optimizer_f", "optimizer_d"])
    assert ck["args"].net == "drn_d_22" and hasattr(ck["args"], "res")
    keys = json.loads(str(fx["keys"]))
    assert list(ck["d_state_dict"]) == [k for k, _ in keys]
    for k, shape in keys:  # 96 x 64 -> a 12 x 8 score map -> 3 x 2 after the two poolings
        own = {"fc1.weight": [10, 6], "conv1.conv1.weight": [10, ck["args"].n_class, 3, 3]}  # (the golden keys are a 5-class classifier's)
        assert list(ck["d_state_dict"][k].shape) == own.get(k, shape), k
    assert all(torch.isfinite(v).all() for sd in ("g_state_dict", "f1_state_dict", "d_state_dict") for v in ck[sd].values() if v.dtype.is_floating_point)
    steps = int(ck["d_state_dict"]["bn1.num_batches_tracked"]) // 4  # two updates, two domains each
    assert steps >= 1 and int(ck["d_state_dict"]["bn1.num_batches_tracked"]) == 4 * steps
    assert all(ck[k]["param_groups"][0]["lr"] == 0.004 for k in ("optimizer_g", "optimizer_f", "optimizer_d"))  # (epoch 0 of 1: no decay yet)
    assert "iter [0] DLoss:" in capsys.readouterr().out
    # resume: continues from epoch 1, and D and its optimizer come back (the reference forgets both)
    ck["args"].epochs = 2
    util.save_checkpoint(ck, False, ck_fn)
    assert dann_trainer.main(["suncg", "nyu", "--resume", ck_fn] + flags) == 0
    ck2 = util.load_checkpoint(os.path.join(pth, "DANN-normal-drn_d_22-2.pth.tar"))
    assert ck2["epoch"] == 2 and int(ck2["d_state_dict"]["bn1.num_batches_tracked"]) == 8 * steps
    # --adjust_lr at epoch 1 of 2 (>= half): G's rate decays by weight_decay, F's by that again (the reference passes the adjusted
    # args.lr on, dann_trainer.py:340-342) -- and D keeps its rate
    wd = ck["args"].weight_decay
    assert ck2["optimizer_g"]["param_groups"][0]["lr"] == pytest.approx(0.004 * wd, rel=1e-9)
    assert ck2["optimizer_f"]["param_groups"][0]["lr"] == pytest.approx(0.004 * wd * wd, rel=1e-9)
    assert ck2["optimizer_d"]["param_groups"][0]["lr"] == 0.004
    assert not torch.equal(ck2["d_state_dict"]["fc2.weight"], ck["d_state_dict"]["fc2.weight"])
    # the MCD tester evaluates the checkpoint as it is
    label_dir, ave_ent = adapt_tester.main(["nyu", ck_fn, "--synthetic", "--synthetic_len", "2", "--outdir", str(tmp_path / "test"),
                                            "--test_img_shape", "80", "56"])[:2]
    names = sorted(os.listdir(label_dir))
    assert len(names) == 2 and all(Image.open(os.path.join(label_dir, n)).size == (80, 56) for n in names)
