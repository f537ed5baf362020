"""The small kernels at the two ends of the DQN and A3C updates, each against a float64 reference of the
same operation (tests/update_refs.py, checked on the CPU by test_update_kernels_host.py): the Huber
loss and gradient, Adam, the Q head, the returns / segments / segment statistics at awkward T, TF1
RMSProp, the TD target and the action draw.

Conventions (test_ntuple_gpu.py's): every output is a slice of a poisoned buffer whose guard is
checked, inputs are compared with their originals after the call, every row is checked, and each
test prints its worst error / bound ratio. u = 2^-24 is fp32's unit roundoff; a bound is a count of
fp32 roundings times the magnitudes involved, stated in the test's docstring.

Sizes are the smallest that reach the code in question: the second grid-stride pass of k_huber_grad
(n > 65,536), of k_adam (n / 4 > 256 * 4096) and of the head's kernels (B > 32 CUs backward, B > 64 CUs
forward), the T % 4 and T % 8 tails of the returns and segment kernels, and single rows.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import update_refs as U
from oracle import a3c_ref as R
from oracle import dqn_ref as D
from test_ntuple_gpu import guard_ok, guarded

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
u = U.U
F32 = np.float32


def lib():
    from rein48_amd import _lib
    return _lib.load()


def check(status):
    from rein48_amd import _lib
    return _lib.check(status)


def ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def stream():
    return C.c_void_p(torch.cuda.current_stream(torch.device(DEV)).cuda_stream)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


def filled(src, fill, row=1):
    """A guarded buffer (raw, view) holding the values of the numpy array src."""
    t = dev(src)
    raw, view = guarded(t.shape[0], t.dtype, fill, row=row)
    view.copy_(t.view(view.shape))
    return raw, view


def shifted(t, fill=0):
    """(raw, view): the values of t in a view that starts 4 bytes (one element) into raw, GUARD after it."""
    k = t.numel()
    raw = torch.full((k + 1 + 256,), fill, dtype=t.dtype, device=DEV)
    raw[1:1 + k] = t.reshape(-1)
    return raw, raw[1:1 + k].view(t.shape)


def shifted_ok(raw, k, fill):
    return bool(raw[0] == fill) and bool((raw[1 + k:] == fill).all())


def report(name, ratio):
    print("%s: worst error / bound = %.3g" % (name, ratio))
    return ratio


def worst(err, bound):
    """max of err / bound over the entries, 0 / 0 counting as 0."""
    err, bound = np.asarray(err, np.float64), np.asarray(bound, np.float64)
    assert not np.isnan(err).any()
    r = np.where(err == 0, 0.0, err / np.where(bound > 0, bound, 1.0))
    r = np.where((err > 0) & (bound <= 0), np.inf, r)
    return float(r.max()) if r.size else 0.0


def close_ratio(got, want, rtol, atol):
    """np.testing.assert_allclose's criterion as a ratio."""
    want = np.asarray(want, np.float64)
    return worst(np.abs(np.asarray(got, np.float64) - want), atol + rtol * np.abs(want))


# ----------------------------------------------------------------------------------- 1. Huber
HUBER_SIZES = [1, 255, 256, 257, 65_535, 65_536, 65_537, 200_003]
_ONE = F32(1)
_BELOW, _ABOVE = np.nextafter(_ONE, F32(0)), np.nextafter(_ONE, F32(2))
PLANTED = np.array([0, 1, -1, _BELOW, -_BELOW, _ABOVE, -_ABOVE, 1e6, -1e6, 1e-20, -1e-20], F32)


def huber_case(n, seed, pool=(0, 1, 2, 3)):
    """q [n, 4], action bytes [n] drawn from pool, y [n]: q_a and y ~ N(0, 2^2); the planted rows have
    y = 0 and q_a = the planted d, so d is exact; the three other Q of a row are +-1e30."""
    rng = np.random.default_rng(seed)
    y = rng.normal(scale=2.0, size=n).astype(F32)
    qa = rng.normal(scale=2.0, size=n).astype(F32)
    if n >= 255:
        rows = np.linspace(0, n - 1, PLANTED.size).astype(np.int64)       # first and last row among them
        y[rows], qa[rows] = 0.0, PLANTED
    act = rng.choice(np.array(pool, np.int8), size=n)
    act[:min(n, len(pool))] = np.array(pool, np.int8)[:min(n, len(pool))]
    code = act.astype(np.int64) & 3
    q = rng.choice(np.array([-1e30, 1e30], F32), size=(n, 4))
    q[np.arange(n), code] = qa
    return q, act, y, code, qa


def huber_call(q, act, y, n):
    tq, ta, ty = dev(q), dev(act), dev(y)
    rd, dq = guarded(n, torch.float32, 7.5, row=4)
    ro, out = guarded(2, torch.float32, 7.5)
    rw, ws = guarded(512, torch.float32, 7.5)
    ws.fill_(float("nan"))
    check(lib().r48_huber_grad(ptr(tq), ptr(ta), ptr(ty), n, ptr(dq), ptr(out), ptr(ws), stream()))
    got = host(dq), host(out), host(ws)
    assert guard_ok(rd, 4 * n, 7.5) and guard_ok(ro, 2, 7.5) and guard_ok(rw, 512, 7.5)
    assert torch.equal(tq, dev(q)) and torch.equal(ta, dev(act)) and torch.equal(ty, dev(y))
    return got


def huber_verify(n, q, act, y, code, qa, name):
    dq, out, ws = huber_call(q, act, y, n)
    d = qa.astype(np.float64) - y.astype(np.float64)
    loss, grad = U.huber(qa, y)
    on = np.zeros((n, 4), bool)
    on[np.arange(n), code] = True
    assert (bits(dq)[~on] == 0).all(), "dq off the action must be +0"
    g = dq[on].astype(np.float64)
    r_dq = worst(np.abs(g - grad), 4 * u * np.abs(grad))
    sat = np.abs(d) >= 1.0 + 2.0 ** -22
    unit = _ONE / F32(n)
    assert (bits(dq[on][sat]) == bits(np.where(d[sat] > 0, unit, -unit).astype(F32))).all()
    count = (-(-n // 65_536) + 12) * u * (1.0 + 2.0 ** -16)
    r_loss = worst(abs(float(out[0]) - loss.mean()), count * loss.mean())
    r_q = worst(abs(float(out[1]) - qa.astype(np.float64).mean()), count * np.abs(qa.astype(np.float64)).mean())
    nb = min(-(-n // 256), 256)
    assert np.isfinite(out).all() and np.isfinite(ws[:2 * nb]).all()
    assert np.isnan(ws[2 * nb:]).all(), "only the 2 partials per block may be written"
    dq2, out2, ws2 = huber_call(q, act, y, n)
    assert (bits(dq) == bits(dq2)).all() and (bits(out) == bits(out2)).all() and (bits(ws) == bits(ws2)).all()
    report("%s n=%d dq" % (name, n), r_dq)
    report("%s n=%d loss" % (name, n), r_loss)
    report("%s n=%d mean q" % (name, n), r_q)
    assert r_dq <= 1 and r_loss <= 1 and r_q <= 1
    return sat


@pytest.mark.parametrize("n", HUBER_SIZES)
def test_huber_loss_and_gradient_match_float64(n):
    """r48_huber_grad against update_refs.huber on every row.
      dq off the action: +0 bits. On the action: within 4 u |ref| of clamp(d, -1, 1) / n -- d = q_a - y,
        inv_n = 1 / n and their product round once each (3 roundings). Where |d| >= 1 + 2^-22 the clamp
        gives exactly +-1, so dq is bit-equal to +-(1 / n) in fp32.
      out[0]: within (ceil(n / 65,536) + 12) u (1 + 2^-16) of the float64 mean loss, relative (the terms
        are non-negative): 3 roundings per term (d twice in d^2, the product or the subtraction), one
        per pass of the lane's running sum (256 x 256 lanes: ceil(n / 65,536) passes), 8 levels of the
        LDS tree, the finish in double and its cast to fp32.
      out[1]: the same count times mean |q_a|.
      The 512-float workspace is NaN before the call: only the 2 partials per block launched may be
      written, and out is finite, so nothing else was read. A second call gives the same bits."""
    q, act, y, code, qa = huber_case(n, 100 + n)
    sat = huber_verify(n, q, act, y, code, qa, "huber")
    if n > 65_536:
        assert n > 256 * 256                                  # the grid-stride loop makes a second pass
    if n >= 255:
        assert sat.sum() >= 4 and sorted(set(code.tolist())) == [0, 1, 2, 3]


def test_huber_takes_the_action_bytes_two_low_bits():
    """Action bytes outside 0..3 select action & 3: 4 and -128 column 0, 7 and -1 column 3."""
    n = 257
    q, act, y, code, qa = huber_case(n, 7, pool=(4, 7, -1, -128))
    assert set(act.tolist()) == {4, 7, -1, -128} and set(code.tolist()) == {0, 3}
    huber_verify(n, q, act, y, code, qa, "huber bytes")


def test_huber_refuses_bad_arguments_and_writes_nothing():
    from rein48_amd import _lib
    n = 8
    q, act, y, _, _ = huber_case(n, 3)
    tq, ta, ty = dev(q), dev(act), dev(y)
    rd, dq = guarded(n, torch.float32, 7.5, row=4)
    ro, out = guarded(2, torch.float32, 7.5)
    rw, ws = guarded(512, torch.float32, 7.5)
    sq_raw, sq = shifted(tq)
    sd_raw, sd = shifted(dq, fill=7.5)
    L = lib()
    assert L.r48_huber_grad(ptr(tq), ptr(ta), ptr(ty), 0, ptr(dq), ptr(out), ptr(ws), stream()) == _lib.R48_EINVAL
    assert L.r48_huber_grad(ptr(sq), ptr(ta), ptr(ty), n, ptr(dq), ptr(out), ptr(ws), stream()) == _lib.R48_EINVAL
    assert L.r48_huber_grad(ptr(tq), ptr(ta), ptr(ty), n, ptr(sd), ptr(out), ptr(ws), stream()) == _lib.R48_EINVAL
    torch.cuda.synchronize()
    assert guard_ok(rd, 0, 7.5) and guard_ok(ro, 0, 7.5) and guard_ok(rw, 0, 7.5)
    assert bool((sd_raw == 7.5).all())


# ------------------------------------------------------------------------------------ 2. Adam
LR, B1, B2, EPS = (float(F32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))      # the values the C-ABI receives
ADAM_BIG = 4 * (256 * 4096) + 12
ADAM_K = 16


def adam_state(n, seed):
    """p, m, v after 3 float64 Adam steps from N(0, 1) parameters, as fp32; every 7th entry has
    m = v = 0 (and g = 0 in every step: `zero`)."""
    rng = np.random.default_rng(seed)
    p, m, v = rng.normal(size=n), np.zeros(n), np.zeros(n)
    for t in range(1, 4):
        p, m, v = U.adam(p, rng.normal(size=n), m, v, t, LR, B1, B2, EPS)
    zero = np.zeros(n, bool)
    zero[::7] = True
    m[zero] = v[zero] = 0.0
    return rng, p.astype(F32), m.astype(F32), v.astype(F32), zero


def adam_grad(rng, n, zero):
    g = rng.normal(size=n)
    kind = rng.integers(0, 10, n)
    for k, val in enumerate((0.0, 1e-12, -1e-12, 1e4, -1e4)):
        g[kind == k] = val
    g[zero] = 0.0
    return g.astype(F32)


def adam_call(bufs, g, n, t):
    tg = dev(g)
    check(lib().r48_adam(ptr(bufs[0][1]), ptr(tg), ptr(bufs[1][1]), ptr(bufs[2][1]), n, LR, B1, B2, EPS, t, stream()))
    torch.cuda.synchronize()
    assert torch.equal(tg, dev(g))
    assert all(guard_ok(raw, n, 7.5) for raw, _ in bufs)
    return tuple(host(view).copy() for _, view in bufs)


def adam_step_check(state, g, got, t, p_ref, spent, zero):
    """One kernel step `got` from the fp32 `state` against update_refs.adam on that state in float64.
    -> (p_ref, spent) advanced and the three ratios."""
    p0, m0, v0 = (a.astype(np.float64) for a in state)
    g64 = g.astype(np.float64)
    dp, m1, v1 = U.adam(np.zeros_like(p0), g64, m0, v0, t, LR, B1, B2, EPS)
    m_mag = np.abs(B1 * m0) + np.abs((1.0 - B1) * g64)
    spent = spent + (LR / (1.0 - B1 ** t)) * m_mag / (np.sqrt(v1 / (1.0 - B2 ** t)) + EPS)
    p_ref = p_ref + dp
    p, m, v = got
    r_m = worst(np.abs(m - m1), 3 * u * m_mag)
    r_v = worst(np.abs(v - v1), 4 * u * v1)
    r_p = worst(np.abs(p - p_ref), ADAM_K * u * (np.abs(p_ref) + spent))
    for a, b in zip(state, got):
        assert (bits(a[zero]) == bits(b[zero])).all(), "g = m = v = 0 must leave p, m and v as they are"
    return p_ref, spent, r_p, r_m, r_v


@pytest.mark.parametrize("n", [4, 1020, 1024])
def test_adam_six_chained_steps_match_float64(n):
    """r48_adam steps 1..6, the kernel's own fp32 state fed back in, against update_refs.adam on that
    state; the float64 p runs along from the start. Gradients: N(0, 1), exact zeros, +-1e-12, +-1e4.
    Bounds (adam_step_check), per step from the kernel's own fp32 state (b1, b2, lr, eps as the fp32
    values the C-ABI receives; 1 - b1 and 1 - b2 are exact in fp32):
      m within 3 u (|b1 m| + |(1 - b1) g|): two products and their sum.
      v within 4 u v': b2 v, (1 - b2) g, its product with g, the sum; all terms non-negative.
      p within K u (|p| + sum over the steps of D), D = (lr / c1) (|b1 m| + |(1 - b1) g|) / (sqrt(v' / c2)
        + eps) -- |dp| with m' taken over the magnitudes of its two addends, which is what m's own
        rounding is relative to. Roundings that reach dp: lr / c1, c2, v' / c2, the square root, + eps
        (together <= 3 u of the denominator), v' (4 u, halved by the root), m' (3 u of the magnitudes),
        the quotient, the product: 11; the subtraction rounds once per step relative to |p|, 6 in 6
        steps, and |p| moved by at most the later D. K = 16 covers both; K u = 9.6e-7 is below the
        rtol 1e-6 of test_fused_adam_matches_torch_adam."""
    rng, p, m, v, zero = adam_state(n, 200 + n)
    bufs = [filled(a, 7.5) for a in (p, m, v)]
    state, p_ref, spent = (p, m, v), p.astype(np.float64), np.zeros(n)
    top = [0.0, 0.0, 0.0]
    for t in range(1, 7):
        g = adam_grad(rng, n, zero)
        got = adam_call(bufs, g, n, t)
        p_ref, spent, *r = adam_step_check(state, g, got, t, p_ref, spent, zero)
        top = [max(a, b) for a, b in zip(top, r)]
        state = got
    for name, r in zip(("p", "m", "v"), top):
        assert report("adam n=%d %s" % (n, name), r) <= 1
    assert ADAM_K * u <= 1e-6


def test_adam_second_grid_stride_pass_with_a_ragged_tail():
    """n = 4 (256 * 4096) + 12 floats: the 4096 x 256 lanes make a second pass over 3 float4s. One
    step (t = 3), every entry checked against float64 with the bounds of the chained test."""
    n = ADAM_BIG
    assert n % 4 == 0 and n // 4 > 256 * 4096
    rng, p, m, v, zero = adam_state(n, 5)
    bufs = [filled(a, 7.5) for a in (p, m, v)]
    g = adam_grad(rng, n, zero)
    got = adam_call(bufs, g, n, 3)
    _, _, r_p, r_m, r_v = adam_step_check((p, m, v), g, got, 3, p.astype(np.float64), np.zeros(n), zero)
    for name, r in zip(("p", "m", "v"), (r_p, r_m, r_v)):
        assert report("adam n=%d %s" % (n, name), r) <= 1


@pytest.mark.parametrize("t", [1000, 10 ** 6])
def test_adam_large_step_counts(t):
    """Single steps where the bias corrections go to 1 (c1 = 1 - 0.9^t is 1 in double from t = 349 on,
    c2 = 1 - 0.999^t is 0.632 at t = 1000 and 1 at 10^6), from given m and v; bounds as above."""
    n = 1020
    rng, p, m, v, zero = adam_state(n, 300)
    bufs = [filled(a, 7.5) for a in (p, m, v)]
    g = adam_grad(rng, n, zero)
    got = adam_call(bufs, g, n, t)
    _, _, r_p, r_m, r_v = adam_step_check((p, m, v), g, got, t, p.astype(np.float64), np.zeros(n), zero)
    assert 1.0 - B1 ** t == 1.0
    for name, r in zip(("p", "m", "v"), (r_p, r_m, r_v)):
        assert report("adam t=%d %s" % (t, name), r) <= 1


def test_adam_refuses_bad_arguments_and_writes_nothing():
    from rein48_amd import _lib
    rng, p, m, v, zero = adam_state(8, 9)
    g = adam_grad(rng, 8, zero)
    bufs = [filled(a, 7.5) for a in (p, g, m, v)]
    before = [raw.clone() for raw, _ in bufs]
    tp, tg, tm, tv = (view for _, view in bufs)
    L = lib()

    def call(a, b, c, d, n, t):
        return L.r48_adam(ptr(a), ptr(b), ptr(c), ptr(d), n, LR, B1, B2, EPS, t, stream())
    assert call(tp, tg, tm, tv, 6, 1) == _lib.R48_EINVAL                  # n % 4 != 0
    assert call(tp, tg, tm, tv, 8, 0) == _lib.R48_EINVAL                  # step < 1
    for k in range(4):                                                     # one pointer 4 bytes off
        args = [tp, tg, tm, tv]
        args[k] = args[k][1:]
        assert call(*args, 4, 1) == _lib.R48_EINVAL
    torch.cuda.synchronize()
    assert all(torch.equal(raw, b) for (raw, _), b in zip(bufs, before))


@pytest.mark.parametrize("fan_in,fused", [(3, True), (4, False)])
def test_trainer_adam_both_forms_agree_with_torch_adam(fan_in, fused):
    """trainer.Adam runs r48_adam when the flat buffer holds a multiple of 4 floats (a Linear(3, 1):
    4) and its torch form otherwise (a Linear(4, 1): 5). Both equal torch.optim.Adam over 6 steps
    within test_fused_adam_matches_torch_adam's rtol 1e-6 / atol 1e-7."""
    from rein48_amd.a3c.optim import FlatParams
    from rein48_amd.dqn.trainer import Adam
    torch.manual_seed(11 + fan_in)
    a = torch.nn.Linear(fan_in, 1).to(DEV)
    b = torch.nn.Linear(fan_in, 1).to(DEV)
    b.load_state_dict(a.state_dict())
    flat = FlatParams(a)
    assert (flat.data.numel() % 4 == 0) == fused and flat.data.numel() == fan_in + 1
    start = host(flat.data).copy()
    mine, ref = Adam(flat, lr=1e-3), torch.optim.Adam(b.parameters(), lr=1e-3)
    for _ in range(6):
        x = torch.randn(32, fan_in, device=DEV)
        flat.zero_grad()
        a(x).square().sum().backward()
        mine.step()
        ref.zero_grad()
        b(x).square().sum().backward()
        ref.step()
    got = np.concatenate([host(a.weight.detach()).ravel(), host(a.bias.detach())])
    want = np.concatenate([host(b.weight.detach()).ravel(), host(b.bias.detach())])
    r = report("trainer.Adam %s form" % ("kernel" if fused else "torch"), close_ratio(got, want, 1e-6, 1e-7))
    assert r <= 1 and (got != start).all()                    # and every parameter has moved


# ---------------------------------------------------------------------------------- 3. Q head
def head_sizes():
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    return cus, [1, 3, 4, 5, 31, 33, 32 * cus + 5, 64 * cus + 3]


@pytest.mark.parametrize("k", range(8))
def test_q_head_forward_and_backward_match_float64(k):
    """r48_q_head_forward / _backward at B = head_sizes()[k] against float64 of the operands the
    kernels use: h bf16, w fp32 rounded to bf16 as QHead rounds it, the bias and dq rounded to bf16
    as the header states. Row B - 1 of h and dq is scaled by 64: a dropped or doubled last row moves
    dw and db far beyond their bound.
      Output rounding: q, dh, dw and db hold bf16 values (bf16 storage or bf16-rounded fp32, as QHead
        returns them): half a bf16 ulp of the value's own binade, update_refs.bf16_half_ulp. bf16 keeps
        8 significant bits, so that is between 2^-9 |x| (top of a binade) and 2^-8 |x| (bottom: 1 + 2^-8
        rounds to 1), and 2^-9 |x| alone does not bound a correct rounding.
      q:  + 1024 u sum_k |h_k w_k| (the products are exact in fp32; 16 fused adds per lane, 6 wave
          levels, the bias: the count of addends bounds any order).
      dh: + 4 u sum_a |dq_a w_a| (4 fused multiply-adds).
      dw, db: + B u sum_b |addend| -- B addends; the longest chain of additions is the lane's boards
          (at most B), then 8 waves and the records, far below B at the large sizes.
    The backward gives the same bits on a second call; the forward too."""
    cus, sizes = head_sizes()
    B = sizes[k]
    if k == 6:
        assert 32 * cus < B <= 64 * cus                       # the backward's second sweep, ragged
    if k == 7:
        assert B > 64 * cus                                   # the forward's second sweep, ragged
    gen = torch.Generator(device="cpu").manual_seed(400 + k)
    h = torch.randn(B, 1024, generator=gen).to(torch.bfloat16)
    w = torch.randn(4, 1024, generator=gen) * 0.05
    bias = torch.randn(4, generator=gen)
    dq = torch.randn(B, 4, generator=gen)
    h[B - 1] *= 64
    dq[B - 1] *= 64
    th, tdq, tb = h.to(DEV), dq.to(DEV), bias.to(DEV)
    wb = w.to(DEV).detach().to(torch.bfloat16).contiguous()   # conv.py q_head_forward / q_head_backward
    keep = [t.clone() for t in (th, tdq, tb, wb)]
    rq, q = guarded(B, torch.float32, 7.5, row=4)
    rh, dh = guarded(B, torch.bfloat16, 7.5, row=1024)
    rg, g = guarded(4 * 1024 + 4, torch.float32, 7.5)
    L = lib()
    ws = torch.empty(int(L.r48_q_head_workspace_floats()), dtype=torch.float32, device=DEV)

    def run():
        check(L.r48_q_head_forward(ptr(th), B, ptr(wb), ptr(tb), ptr(q), stream()))
        check(L.r48_q_head_backward(ptr(tdq), ptr(th), B, ptr(wb), ptr(dh), ptr(ws), ptr(g), stream()))
        return host(q).copy(), host(dh.float()).copy(), host(g).copy()
    got_q, got_dh, got_g = run()
    assert guard_ok(rq, 4 * B, 7.5) and guard_ok(rh, 1024 * B, 7.5) and guard_ok(rg, 4100, 7.5)
    assert all(torch.equal(a, b) for a, b in zip((th, tdq, tb, wb), keep))
    ref = U.q_head(h.double().numpy(), wb.double().cpu().numpy(), bias.to(torch.bfloat16).double().numpy(),
                   dq.to(torch.bfloat16).double().numpy())
    assert (got_q == host(q.to(torch.bfloat16).float())).all() and (got_g == host(g.to(torch.bfloat16).float())).all()

    def ratio(got, want, e32):
        return worst(np.abs(got - want), U.bf16_half_ulp(np.abs(want) + e32) + e32)
    r = {"q": ratio(got_q, ref["q"], 1024 * u * ref["q_mag"]),
         "dh": ratio(got_dh, ref["dh"], 4 * u * ref["dh_mag"]),
         "dw": ratio(got_g[:4096].reshape(4, 1024), ref["dw"], B * u * ref["dw_mag"]),
         "db": ratio(got_g[4096:], ref["db"], B * u * ref["db_mag"])}
    again = run()
    assert (bits(got_q) == bits(again[0])).all() and (bits(got_dh) == bits(again[1])).all()
    assert (bits(got_g) == bits(again[2])).all()
    for name, val in r.items():
        assert report("q head B=%d %s" % (B, name), val) <= 1
    if B == 5:      # QHead returns these bits: fp32 q, bf16 dh, bf16-rounded fp32 dw and db
        from rein48_amd.dqn.conv import QHead
        hh = th.clone().requires_grad_(True)
        wp, bp = w.to(DEV).requires_grad_(True), tb.clone().requires_grad_(True)
        out = QHead.apply(hh, wp, bp)
        out.backward(tdq)
        assert out.dtype == torch.float32 and hh.grad.dtype == torch.bfloat16
        assert wp.grad.dtype == torch.float32 and bp.grad.dtype == torch.float32
        assert (host(out.detach()) == got_q).all() and (host(hh.grad.float()) == got_dh).all()
        assert (host(wp.grad).ravel() == got_g[:4096]).all() and (host(bp.grad) == got_g[4096:]).all()


# --------------------------------------------------- 4. returns, segments, segment statistics
RET_T = [1, 2, 3, 5, 6, 7, 8, 9, 13, 15, 16, 17]
RET_N = [4, 8, 260]
GAMMA = 0.9


def ret_case(T, n, seed):
    rng = np.random.default_rng(seed)
    special = [-2, 0, 1, 2, T - 1, T, T + 3]
    lengths = rng.integers(0, T + 1, n)
    k = min(n, 7) if n > 4 else 4
    lengths[:k] = [special[(T + j) % 7] for j in range(k)]    # n = 4: four of the seven, rotating with T
    if n >= 14:
        lengths[-7:] = special                                # the last lanes as well
    return (rng.normal(size=(T, n)).astype(F32), lengths.astype(np.int32), rng.normal(size=n).astype(F32),
            rng.normal(size=(T, n)).astype(F32), rng.integers(0, 4, (T, n)).astype(np.int8))


def returns_call(rw, ln, bt, T, n, drop_last, out):
    check(lib().r48_discounted_returns(ptr(rw), ptr(ln), ptr(bt), T, n, GAMMA, int(drop_last), ptr(out), stream()))
    return host(out).copy()


@pytest.mark.parametrize("T", RET_T)
def test_returns_segments_and_stats_at_awkward_lengths(T):
    """T around the 4-row groups of k_returns4 and the 8-row groups of k_returns, k_segments and
    k_segment_stats (T < 8, T = 0, 1, 7 mod 8), n = 4, 8 and 260 (one lane, two lanes, two workgroups
    of the scalar path), both drop_last settings. Lengths -2, 0, 1, 2, T - 1, T, T + 3 and uniform
    0..T; they count as clamp(len, 0, T).
      r48_discounted_returns: the float4 path (aligned, n % 4 == 0) and the scalar path (4-byte-offset
        views) are bit-equal; both within rtol 1e-5 / atol 1e-5 (test_discounted_returns_match_oracle's)
        of update_refs.returns on every column; rows t >= L are exactly 0.
      r48_a3c_segments: targets bit-equal to the returns; seg = {(1 / max(L, 1)) (1 / n) in fp32, c0, L
        as int32 bits, 0}; counts = a numpy bincount over t < L; c0 bit-equal to r48_a3c_row_weights' cm
        from r48_a3c_segment_stats' td_sum (0 for an empty segment, and without values / actions).
      r48_a3c_segment_stats: B = max(L, 1) and the counts exact; td_sum within L u sum |target - value|
        of the float64 sum (each difference rounds once, u sum |.| in all, and L - 1 additions follow),
        below the 1e-5 of the T = 100 test."""
    from rein48_amd.a3c import kernels as K
    L_ = lib()
    top = {"returns": 0.0, "td_sum": 0.0}
    for n in RET_N:
        rewards, lengths, boot, values, actions = ret_case(T, n, 1000 * T + n)
        Lc = np.clip(lengths, 0, T)
        valid = np.arange(T)[:, None] < Lc[None, :]
        tr, tl, tb, tv, ta = dev(rewards), dev(lengths), dev(boot), dev(values), dev(actions)
        keep = [t.clone() for t in (tr, tl, tb, tv, ta)]
        for drop_last in (True, False):
            want = U.returns(rewards, lengths, boot, GAMMA, drop_last)
            ro, out = guarded(T, torch.float32, 7.5, row=n)
            got4 = returns_call(tr, tl, tb, T, n, drop_last, out)
            assert guard_ok(ro, T * n, 7.5)
            (_, sr), (_, sl), (_, sb) = shifted(tr), shifted(tl), shifted(tb)
            so_raw, so = shifted(torch.empty(T, n, device=DEV), fill=7.5)
            got1 = returns_call(sr, sl, sb, T, n, drop_last, so)
            assert shifted_ok(so_raw, T * n, 7.5)
            assert (bits(got4) == bits(got1)).all(), "float4 path != scalar path"
            assert (got4[~valid] == 0).all()
            top["returns"] = max(top["returns"], close_ratio(got4, want, 1e-5, 1e-5))
            # the fused per-board pass, with and without the reference loss's values / actions
            for td in (True, False):
                rt, tg = guarded(T, torch.float32, 7.5, row=n)
                rs, seg = guarded(n, torch.float32, 7.5, row=4)
                rc, cnt = guarded(n, torch.float32, 7.5, row=4)
                check(L_.r48_a3c_segments(ptr(tr), ptr(tv) if td else None, ptr(ta) if td else None, ptr(tl), ptr(tb),
                                          T, n, GAMMA, int(drop_last), ptr(tg), ptr(seg), ptr(cnt) if td else None,
                                          stream()))
                s = host(seg).copy()
                assert guard_ok(rt, T * n, 7.5) and guard_ok(rs, 4 * n, 7.5) and guard_ok(rc, 4 * n if td else 0, 7.5)
                assert (bits(host(tg)) == bits(got4)).all()
                assert (bits(s[:, 2]) == Lc).all() and (bits(s[:, 3]) == 0).all()
                w0 = (_ONE / np.maximum(Lc, 1).astype(F32)) * (_ONE / F32(n))
                assert w0.dtype == F32 and (bits(s[:, 0]) == bits(w0)).all()
                if not td:
                    assert (bits(s[:, 1]) == 0).all()
                    continue
                bins = np.stack([((actions == a) & valid).sum(0) for a in range(4)], 1)
                assert (host(cnt) == bins).all()
                # r48_a3c_segment_stats on the same targets
                rB, Bv = guarded(n, torch.float32, 7.5)
                rtd, tds = guarded(n, torch.float32, 7.5)
                rc2, cnt2 = guarded(n, torch.float32, 7.5, row=4)
                check(L_.r48_a3c_segment_stats(ptr(tv), ptr(tg), ptr(ta), ptr(tl), T, n, ptr(Bv), ptr(tds), ptr(cnt2),
                                               stream()))
                assert guard_ok(rB, n, 7.5) and guard_ok(rtd, n, 7.5) and guard_ok(rc2, 4 * n, 7.5)
                assert (host(Bv) == np.maximum(Lc, 1)).all() and (host(cnt2) == bins).all()
                diff = (got4.astype(np.float64) - values.astype(np.float64)) * valid
                top["td_sum"] = max(top["td_sum"], worst(np.abs(host(tds) - diff.sum(0)), Lc * u * np.abs(diff).sum(0)))
                _, cm = K.row_weights(dev(Lc.astype(np.int32)), Bv.contiguous(), T, tds.contiguous())
                cm = host(cm)
                assert (cm[~valid] == 0).all()
                assert (bits(cm)[valid] == bits(np.broadcast_to(s[:, 1], (T, n)).copy())[valid]).all()
                assert (bits(s[Lc == 0, 1]) & 0x7FFFFFFF == 0).all()
        assert all(torch.equal(a, b) for a, b in zip((tr, tl, tb, tv, ta), keep))
    report("returns T=%d" % T, top["returns"])
    report("segment_stats td_sum T=%d" % T, top["td_sum"])
    assert top["returns"] <= 1 and top["td_sum"] <= 1


# ------------------------------------------------------------- 5. RMSProp, TD target, sampling
@pytest.mark.parametrize("n", [1, 255, 257, 40_001])
@pytest.mark.parametrize("decay,momentum,eps", [(0.9, 0.0, 1e-10), (0.99, 0.9, 1e-3)])
def test_rmsprop_five_chained_steps_match_float64(n, decay, momentum, eps):
    """r48_rmsprop_tf1 over 5 chained steps against oracle.a3c_ref.rmsprop_tf1 in float64 (its own
    float64 chain, the constants as the fp32 values the kernel receives): var, ms and mom within
    test_rmsprop_kernel_matches_oracle's rtol 1e-5 / atol 1e-6 after every step. Every 5th gradient is
    0: with momentum 0 such a step leaves var bit-identical."""
    from rein48_amd.a3c import kernels as K
    rng = np.random.default_rng(500 + n)
    lr, dc, mo, ep = (float(F32(x)) for x in (1e-3, decay, momentum, eps))
    var, ms, mom = rng.normal(size=n).astype(F32).astype(np.float64), np.ones(n), np.zeros(n)
    bufs = [filled(a.astype(F32), 7.5) for a in (var, ms, mom)]
    top = 0.0
    for step in range(5):
        g = rng.normal(size=n).astype(F32)
        g[(np.arange(n) + step) % 5 == 0] = 0.0
        before = host(bufs[0][1]).copy()
        tg = dev(g)
        K.rmsprop_tf1_(bufs[0][1], tg, bufs[1][1], bufs[2][1], lr, decay=dc, momentum=mo, eps=ep)
        var, ms, mom = R.rmsprop_tf1(var, g.astype(np.float64), ms, mom, lr, dc, mo, ep)
        got = [host(view) for _, view in bufs]
        assert torch.equal(tg, dev(g)) and all(guard_ok(raw, n, 7.5) for raw, _ in bufs)
        if momentum == 0.0:
            assert (bits(got[0][g == 0]) == bits(before[g == 0])).all()
        top = max([top] + [close_ratio(a, b, 1e-5, 1e-6) for a, b in zip(got, (var, ms, mom))])
    assert report("rmsprop n=%d momentum=%g" % (n, momentum), top) <= 1


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("with_done", [True, False])
def test_td_target_done_bytes_and_first_online_argmax(double, with_done):
    """r48_td_target at n = 257. Any nonzero done byte (1, 2, 0x80, 0xFF) ends the episode: y is
    bit-equal to the reward (r + gamma 0); the other rows, and every row with done = NULL, are within
    test_td_target_matches_oracle's 1e-6 of oracle.dqn_ref.td_target. Double DQN: the target Q of a row
    are 1, 2, 3, 4 in a random order, so a pick that does not follow the FIRST online argmax (planted
    ties between two and between all four online Q included) misses by at least gamma."""
    n, gamma = 257, float(F32(0.97))
    rng = np.random.default_rng(600 + double)
    r = rng.normal(size=n).astype(F32)
    done = rng.choice(np.array([0, 0, 0, 0, 0, 0, 1, 2, 0x80, 0xFF], np.uint8), size=n)
    done[:6] = [0, 1, 2, 0x80, 0xFF, 0]
    qt = np.stack([rng.permutation(4) + 1.0 for _ in range(n)]).astype(F32)
    qo = rng.normal(size=(n, 4)).astype(F32)
    qo[5::9, 3] = qo[5::9, 1] = qo[5::9].max(1) + 1                       # the online maximum twice
    qo[7::13] = 0.25                                                      # all four equal
    tr, td_, tqt, tqo = dev(r), dev(done), dev(qt), dev(qo)
    ry, y = guarded(n, torch.float32, 7.5)
    check(lib().r48_td_target(ptr(tr), ptr(td_) if with_done else None, ptr(tqt), ptr(tqo) if double else None, n,
                              gamma, 0, ptr(y), stream()))
    got = host(y)
    assert guard_ok(ry, n, 7.5)
    assert torch.equal(tr, dev(r)) and torch.equal(td_, dev(done)) and torch.equal(tqt, dev(qt)) and torch.equal(tqo, dev(qo))
    ended = (done != 0) if with_done else np.zeros(n, bool)
    want = D.td_target(r, ended, qt, qo if double else None, gamma)
    assert ended.sum() >= 4 * with_done and (bits(got[ended]) == bits(r[ended])).all()
    if double:
        differ = qo.argmax(1) != qt.argmax(1)
        tied = (qo == qo.max(1, keepdims=True)).sum(1) > 1
        assert (differ & ~ended).sum() >= 50 and (tied & ~ended).sum() >= 10
    assert report("td target double=%s done=%s" % (double, with_done), close_ratio(got, want, 1e-6, 1e-6)) <= 1


def sample_families(n, rng):
    """Four families of logits [n, 4], all multiples of 1/8: (a) within +-16; (b) the same with column
    i % 4 raised by 120 (the others' probabilities underflow); (c) all four equal; (d) two equal pairs
    in the three possible arrangements."""
    grid = lambda *shape: rng.integers(-128, 129, shape).astype(np.float64) / 8.0
    a = grid(n, 4)
    b = grid(n, 4)
    b[np.arange(n), np.arange(n) % 4] += 120.0
    c = np.repeat(grid(n, 1), 4, axis=1)
    lo, hi = grid(n), grid(n)
    pairs = np.array([[0, 0, 1, 1], [0, 1, 0, 1], [0, 1, 1, 0]])[np.arange(n) % 3]
    d = np.where(pairs == 0, lo[:, None], hi[:, None])
    return {"grid": a, "dominant": b, "equal": c, "pairs": d}


@pytest.mark.parametrize("family", ["grid", "dominant", "equal", "pairs"])
def test_sample_actions_edge_logits(family):
    """r48_sample_actions at n = 70,001 on every row, uniforms from update_refs.sample_uniforms; the
    board ids run across 2^32 inside the batch.
      The action equals oracle.a3c_ref.choose_action wherever u is more than 1e-5 from a cdf boundary;
        those rows are at least 99.9 % of the family.
      logp and the entropy term are within test_sample_actions_match_choose_action's rtol 1e-4 /
        atol 1e-5 of float64.
      Adding 1024 to every logit changes no bit of the action, logp or entropy: the logits are
        multiples of 1/8 below 2^11, so z - max is the same exact number.
      A dominant column (the others' e^(z - max) <= e^-88) is the action drawn whenever u > 0, column
        3 -- reached by falling through the three cdf comparisons -- included."""
    n, seed, gid0, ctr = 70_001, (3 << 32) | 77, 2 ** 32 - 35_000, 0xFFFFFFFF
    z = sample_families(n, np.random.default_rng(700))[family]
    uni = U.sample_uniforms(n, seed, gid0, ctr)

    def run(logits):
        tz = dev(logits.astype(F32))
        ra, act = guarded(n, torch.int8, 0x55)
        rl, logp = guarded(n, torch.float32, 7.5)
        re, ent = guarded(n, torch.float32, 7.5)
        check(lib().r48_sample_actions(ptr(tz), n, seed, gid0, ctr, ptr(act), ptr(logp), ptr(ent), stream()))
        out = host(act).copy(), host(logp).copy(), host(ent).copy()
        assert guard_ok(ra, n, 0x55) and guard_ok(rl, n, 7.5) and guard_ok(re, n, 7.5)
        assert torch.equal(tz, dev(logits.astype(F32)))
        return out
    assert (z.astype(F32).astype(np.float64) == z).all() and ((z + 1024).astype(F32).astype(np.float64) == z + 1024).all()
    act, logp, ent = run(z)
    probs = R.softmax(z)
    cdf = np.cumsum(probs, -1)
    far = np.min(np.abs(cdf[:, :3] - uni[:, None]), axis=1) > 1e-5
    print("sample %s: %.4f %% of the rows are away from a cdf boundary" % (family, 100 * far.mean()))
    assert far.mean() >= 0.999
    assert set(act.tolist()) <= {0, 1, 2, 3}
    assert (act[far] == R.choose_action(probs, uni)[far]).all()
    rows = np.arange(n)
    r_lp = close_ratio(logp, np.log(probs[rows, act.astype(np.int64)]), 1e-4, 1e-5)
    r_en = close_ratio(ent, -np.sum(probs * np.log(probs + 1e-5), -1), 1e-4, 1e-5)
    act2, logp2, ent2 = run(z + 1024.0)
    assert (act == act2).all() and (bits(logp) == bits(logp2)).all() and (bits(ent) == bits(ent2)).all()
    if family == "dominant":
        pos = uni > 0
        assert pos.mean() > 0.9999 and (act[pos] == (rows % 4)[pos]).all() and (act[pos] == 3).sum() > n // 5
    if family == "equal":
        assert (act == np.minimum((uni * 4).astype(np.int64), 3)).all()          # p = 1/4 and the cdf are exact
    assert report("sample %s logp" % family, r_lp) <= 1 and report("sample %s entropy" % family, r_en) <= 1
