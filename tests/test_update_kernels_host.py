"""The float64 references of tests/update_refs.py against independent statements of the same maths, on
the CPU: a wrong reference must not be able to agree with a wrong kernel in test_update_kernels_gpu.py.

Huber against torch's smooth_l1_loss and autograd, Adam against torch.optim.Adam, the returns slab
against the reference's own executed outputs (tests/golden/a3c_golden.json), the vectorised Philox
against the C oracle's, the BatchNorm forward and backward (test_bn_kernels_gpu.py's references) against
torch's batch_norm and autograd, the 3x3 conv and its two gradients (test_conv_kernels_gpu.py's
references) against torch's conv2d and autograd. RMSProp and the TD target are oracle/a3c_ref.py's and oracle/dqn_ref.py's,
which test_a3c.py and test_dqn.py cover.
"""
import json
import os

import numpy as np
import pytest
import torch

import update_refs as U
from oracle import native as O


def test_huber_reference_matches_smooth_l1_and_autograd():
    """Loss per row and the gradient of the mean, float64 against float64 (1e-15: the same few
    operations). The planted rows sit on and next to the |d| = 1 switch."""
    rng = np.random.default_rng(0)
    one = np.float32(1)
    planted = [0.0, 1.0, -1.0, float(np.nextafter(one, np.float32(0))), -float(np.nextafter(one, np.float32(0))),
               float(np.nextafter(one, np.float32(2))), -float(np.nextafter(one, np.float32(2))), 1e6, -1e6, 1e-20,
               -1e-20]
    y = rng.normal(scale=2.0, size=1003)
    qa = rng.normal(scale=2.0, size=1003)
    qa[:len(planted)] = y[:len(planted)] + planted
    loss, grad = U.huber(qa, y)
    tq = torch.tensor(qa, dtype=torch.float64, requires_grad=True)
    rows = torch.nn.functional.smooth_l1_loss(tq, torch.tensor(y, dtype=torch.float64), reduction="none")
    rows.mean().backward()
    np.testing.assert_allclose(loss, rows.detach().numpy(), rtol=1e-15, atol=0)
    np.testing.assert_allclose(grad, tq.grad.numpy(), rtol=1e-15, atol=0)
    d = qa - y
    assert (grad[np.abs(d) >= 1] == np.sign(d[np.abs(d) >= 1]) / d.size).all()


def test_adam_reference_matches_torch_adam_over_6_steps():
    """6 chained steps in float64 with zero, tiny and huge gradients: the operation order differs
    (torch divides the step size, not the moment), so 1e-13 relative."""
    rng = np.random.default_rng(1)
    n = 257
    p = rng.normal(size=n)
    tp = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([tp], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    m, v = np.zeros(n), np.zeros(n)
    for t in range(1, 7):
        g = rng.normal(size=n)
        g[::5] = 0.0
        g[1::7] = 1e-12
        g[2::11] = -1e4
        tp.grad = torch.tensor(g, dtype=torch.float64)
        opt.step()
        p, m, v = U.adam(p, g, m, v, t)
        np.testing.assert_allclose(p, tp.detach().numpy(), rtol=1e-13, atol=1e-15)
    st = opt.state[tp]
    np.testing.assert_allclose(m, st["exp_avg"].numpy(), rtol=1e-13, atol=0)
    np.testing.assert_allclose(v, st["exp_avg_sq"].numpy(), rtol=1e-13, atol=0)


def test_adam_reference_leaves_an_all_zero_entry_alone():
    p, m, v = U.adam(np.array([1.5, -2.0]), np.zeros(2), np.zeros(2), np.zeros(2), 3)
    assert (p == [1.5, -2.0]).all() and (m == 0).all() and (v == 0).all()


def test_returns_reference_matches_every_golden_case():
    """All 48 executed reference cases in one slab, ragged lengths: rows below the length equal the
    golden targets (1e-12), rows from the length on are zero."""
    g = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "a3c_golden.json")))["returns"]
    T, n = max(len(c["rewards"]) for c in g) + 2, len(g)
    rewards = np.full((T, n), 7.0)                          # rows past a length must not enter
    for i, c in enumerate(g):
        rewards[:len(c["rewards"]), i] = c["rewards"]
    lengths = [len(c["rewards"]) for c in g]
    boot = [c["last_target_value"] for c in g]
    out = U.returns(rewards, lengths, boot, 0.9, True)
    for i, c in enumerate(g):
        np.testing.assert_allclose(out[:lengths[i], i], c["targets"], rtol=1e-12, atol=1e-12)
        assert (out[lengths[i]:, i] == 0).all()


def test_returns_reference_clamps_lengths_and_knows_both_modes():
    """Hand-computed columns (gamma 0.5, bootstrap 0.5, rewards (i + 1) 10^t: every value exact)."""
    r = np.outer([1.0, 10.0, 100.0], [1.0, 2.0, 3.0, 4.0, 5.0])                              # [T = 3][n = 5]
    out = U.returns(r, [-2, 0, 2, 3, 6], [0.5] * 5, 0.5, True)
    assert (out[:, :2] == 0).all()
    np.testing.assert_array_equal(out[:, 2], [3.25, 0.5, 0.0])
    np.testing.assert_array_equal(out[:, 3], [24.125, 40.25, 0.5])
    np.testing.assert_array_equal(out[:, 4], [30.125, 50.25, 0.5])                           # length 6 counts as 3
    tb = U.returns(r, [-2, 0, 2, 3, 6], [0.5] * 5, 0.5, False)
    assert (tb[:, :2] == 0).all()
    np.testing.assert_array_equal(tb[:, 2], [18.125, 30.25, 0.0])
    np.testing.assert_array_equal(tb[:, 4], [155.0625, 300.125, 500.25])


def test_vectorised_philox_matches_the_oracle():
    """A few hundred counters, board ids above 2^32 and the all-ones counter among them, two keys."""
    rng = np.random.default_rng(2)
    n = 300
    ctr = rng.integers(0, 2 ** 32, size=(n, 4), dtype=np.uint64)
    gid = (2 ** 32 + 5) + np.arange(40, dtype=np.uint64)
    ctr[:40, 0], ctr[:40, 1] = gid & np.uint64(0xFFFFFFFF), gid >> np.uint64(32)
    ctr[40] = 0xFFFFFFFF
    ctr[41] = 0
    for key in ((77, 0), (0xDEADBEEF, 0xFFFFFFFF)):
        got = U.philox4x32_10(ctr, key)
        want = np.stack([O.philox([int(x) for x in row], list(key)) for row in ctr])
        np.testing.assert_array_equal(got, want)


def test_sample_uniforms_follow_the_draw_contract():
    seed, gid0, ctr, n = (5 << 32) | 77, 2 ** 32 - 3, 0xFFFFFFFF, 9
    u = U.sample_uniforms(n, seed, gid0, ctr)
    for i in range(n):
        g = gid0 + i
        w = O.philox([g & 0xFFFFFFFF, g >> 32, ctr, 0xA3C], [seed & 0xFFFFFFFF, seed >> 32])
        assert u[i] == (int(w[0]) >> 8) / 16777216.0 and 0.0 <= u[i] < 1.0


def _bn_host_case(n, C, seed):
    """bf16-valued x, res, g [n, C] and gamma, beta, rm, rv [C] in float64. Channel 1 is constant,
    channel 2 has |mean| / std = 128, gamma is 0 in channel 3 and negative in channel 4."""
    gen = torch.Generator().manual_seed(seed)
    mu, sd = torch.randn(C, generator=gen) * 2, torch.rand(C, generator=gen) + 0.5
    mu[2], sd[2] = 0.998, 0.998 / 128
    x = torch.randn(n, C, generator=gen) * sd + mu
    x[:, 1] = 1.5
    x, res, g = (t.to(torch.bfloat16).double() for t in (x, torch.randn(n, C, generator=gen), torch.randn(n, C, generator=gen)))
    gamma, beta = torch.randn(C, generator=gen).double() + 1, torch.randn(C, generator=gen).double()
    gamma[3], gamma[4] = 0.0, -1.25
    return x, res, g, gamma, beta, torch.randn(C, generator=gen).double(), torch.rand(C, generator=gen).double() + 0.5


@pytest.mark.parametrize("n", [2, 3, 257])
@pytest.mark.parametrize("with_res,relu", [(False, False), (False, True), (True, False), (True, True)])
@pytest.mark.parametrize("momentum,eps", [(0.1, 1e-5), (1.0, 1e-3)])
def test_bn_references_match_torch_batch_norm_and_autograd(n, with_res, relu, momentum, eps):
    """update_refs.bn_forward / bn_backward against torch.nn.functional.batch_norm (training mode)
    + add + ReLU and autograd, float64 on the CPU: rtol 1e-12, with an absolute 1e-13 of the largest
    entry for the entries that cancel to nearly nothing (a constant channel's dgamma is 0 up to the
    last bit of its mean). bn_backward gets the gradient through the ReLU of the reference's own y."""
    C = 8
    x, res, dy, gamma, beta, rm, rv = _bn_host_case(n, C, 10 * n + relu)
    f = U.bn_forward(x.numpy(), res.numpy() if with_res else None, gamma.numpy(), beta.numpy(), rm.numpy(), rv.numpy(),
                     momentum, eps, relu)
    tx, tg, tb = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    tr = res.clone().requires_grad_(True)
    trm, trv = rm.clone(), rv.clone()
    z = torch.nn.functional.batch_norm(tx, trm, trv, tg, tb, True, momentum, eps)
    if with_res:
        z = z + tr
    y = torch.relu(z) if relu else z
    y.backward(dy)

    def close(got, want):
        want = want.detach().numpy() if torch.is_tensor(want) else want
        np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-13 * np.abs(want).max())
    close(f["y"], y)
    close(f["rm"], trm)
    close(f["rv"], trv)
    close(f["mean"], x.mean(0))
    close(f["var"], x.var(0, unbiased=False))
    close(f["z"], f["a"] * x.numpy() + f["b"] + (res.numpy() if with_res else 0.0))
    assert f["var"][1] == 0 and f["mean"][1] == 1.5 and f["invstd"][1] == 1.0 / np.sqrt(eps)
    assert 100 < abs(f["mean"][2]) / np.sqrt(f["var"][2]) < 200 or n < 257
    g = dy.numpy() * (f["y"] > 0) if relu else dy.numpy()
    b = U.bn_backward(g, x.numpy(), f["mean"], f["invstd"], gamma.numpy())
    close(b["dx"], tx.grad)
    close(b["dgamma"], tg.grad)
    close(b["dbeta"], tb.grad)
    if with_res:
        close(g, tr.grad)
    mag = np.abs(b["a"] * g) + np.abs(b["cc"] * x.numpy()) + np.abs(b["d"])
    assert (np.abs(b["a"] * g + b["cc"] * x.numpy() + b["d"] - b["dx"]) <= 1e-14 * mag).all()
    assert b["dgamma"][1] == 0 and (b["dx"][:, 3] == 0).all()
    np.testing.assert_array_equal(b["g_mag"], np.abs(g).sum(0))
    np.testing.assert_array_equal(b["gx_mag"], (np.abs(g) * np.abs(x.numpy() - f["mean"])).sum(0))
    s = U.bn_from_sums(x.numpy().sum(0), np.square(x.numpy()).sum(0), n, 0.0, gamma.numpy(), beta.numpy(), rm.numpy(),
                       rv.numpy(), momentum, eps)
    for k in ("mean", "a", "rm"):                # plain sums lose 128^2 of the variance's digits in channel 2
        np.testing.assert_allclose(s[k], f[k], rtol=1e-12 * (16384 if k == "a" else 1), atol=1e-13)
    np.testing.assert_allclose(s["var"], f["var"], rtol=0, atol=1e-13 * np.square(x.numpy()).mean(0).max())


def test_bn_reference_single_row_takes_the_variance_itself():
    """n = 1: var = 0, and the running variance moves towards var itself (no n / (n - 1))."""
    x = np.array([[1.5, -2.0]])
    f = U.bn_forward(x, None, np.ones(2), np.zeros(2), np.zeros(2), np.ones(2), 0.25, 1e-5, False)
    assert (f["var"] == 0).all() and (f["mean"] == x[0]).all() and (f["rv"] == 0.75).all() and (f["y"] == 0).all()
    assert U.bn_forward(x, None, np.ones(2), np.zeros(2), None, None, 0.25, 1e-5, False)["rm"] is None


def test_bf16_half_ulp_bounds_round_to_nearest():
    """bf16 keeps 8 significant bits: rounding 1 + 2^-8 (a tie, to even: 1) errs by 2^-8, more than
    2^-9 |x|; half an ulp of the value's own binade is the bound that holds everywhere."""
    x = torch.tensor([1.0 + 2.0 ** -8, 1.99, 3.0e-5, 255.5, 1.0e6], dtype=torch.float64)
    x = torch.cat([x, torch.linspace(0.5, 4.0, 9973, dtype=torch.float64)])
    err = (x.float().to(torch.bfloat16).double() - x).abs().numpy()
    hu = U.bf16_half_ulp(x.numpy())
    assert (err <= hu).all() and err[0] == 2.0 ** -8 and err[0] > 2.0 ** -9 * float(x[0])
    assert (hu >= 2.0 ** -9 * x.numpy() * (1 - 1e-15)).all() and (hu <= 2.0 ** -8 * x.numpy()).all()
    assert U.bf16_half_ulp(0.0) == 0.0


@pytest.mark.parametrize("cin", [32, 64])
@pytest.mark.parametrize("as_torch", [False, True])
def test_conv_references_match_conv2d_and_autograd(cin, as_torch):
    """update_refs.conv3x3, conv3x3_dgrad and conv3x3_wgrad at B = 3 against torch.nn.functional.conv2d
    (padding 1) and autograd in float64, on numpy arrays and on torch tensors (the form the GPU tests
    evaluate on the device): 1e-13 of the entry's sum of magnitudes (the same few hundred products in
    another order), and the magnitude sums against the same functions of the absolute values. An
    input that is zero but for one cell / one tap pins the cell and tap indexing on its own."""
    B = 3
    rng = np.random.default_rng(cin)
    x, dy, add = rng.normal(size=(B, 16, cin)), rng.normal(size=(B, 16, 64)), rng.normal(size=(B, 16, 64))
    addx = rng.normal(size=(B, 16, cin))
    w, bias = rng.normal(size=(64, cin, 3, 3)) * 0.1, rng.normal(size=64)
    wrap = torch.from_numpy if as_torch else (lambda a: a)
    back = (lambda a: a.numpy()) if as_torch else (lambda a: a)

    def nchw(a):
        return torch.from_numpy(a).permute(0, 2, 1).reshape(a.shape[0], a.shape[2], 4, 4)

    def cells(t):
        return t.reshape(t.shape[0], t.shape[1], 16).permute(0, 2, 1).detach().numpy()

    def close(got, want, mag):
        assert got.shape == want.shape and (np.abs(got - want) <= 1e-13 * mag).all()
    tx, tw = nchw(x).clone().requires_grad_(True), torch.from_numpy(w).clone().requires_grad_(True)
    ty = torch.nn.functional.conv2d(tx, tw, torch.from_numpy(bias), padding=1)
    ty.backward(nchw(dy))
    for b, a in ((bias, add), (None, None), (bias, None)):
        y, mag = (back(v) for v in U.conv3x3(wrap(x), wrap(w), None if b is None else wrap(b), None if a is None else wrap(a)))
        want = cells(ty) + (0.0 if a is None else a) - (0.0 if b is not None else bias)
        close(y, want, mag)
        m2 = back(U.conv3x3(wrap(np.abs(x)), wrap(np.abs(w)), None if b is None else wrap(np.abs(b)),
                            None if a is None else wrap(np.abs(a)))[0])
        close(mag, m2, m2)
        assert (mag >= np.abs(y)).all()
    dx, mag = (back(v) for v in U.conv3x3_dgrad(wrap(dy), wrap(w), wrap(addx)))
    close(dx, cells(tx.grad) + addx, mag)
    dx0, mag0 = (back(v) for v in U.conv3x3_dgrad(wrap(dy), wrap(w)))
    close(dx0, cells(tx.grad), mag0)
    close(mag, back(U.conv3x3_dgrad(wrap(np.abs(dy)), wrap(np.abs(w)), wrap(np.abs(addx)))[0]), mag)
    dw, mag = (back(v) for v in U.conv3x3_wgrad(wrap(dy), wrap(x)))
    close(dw, tw.grad.numpy(), mag)
    close(mag, back(U.conv3x3_wgrad(wrap(np.abs(dy)), wrap(np.abs(x)))[0]), mag)
    # one non-zero input entry, one non-zero weight: y is that product at the one cell the tap reaches
    for cell, kr, kc in ((0, 0, 0), (3, 1, 2), (5, 2, 0), (15, 2, 2), (12, 0, 1)):
        x1, w1 = np.zeros((1, 16, cin)), np.zeros((64, cin, 3, 3))
        x1[0, cell, cin - 1], w1[7, cin - 1, kr, kc] = 2.0, 3.0
        y1 = back(U.conv3x3(wrap(x1), wrap(w1))[0])
        r, c = cell // 4 - (kr - 1), cell % 4 - (kc - 1)          # the output cell whose tap (kr, kc) reads `cell`
        want = np.zeros((1, 16, 64))
        if 0 <= r < 4 and 0 <= c < 4:
            want[0, 4 * r + c, 7] = 6.0
        np.testing.assert_array_equal(y1, want)
