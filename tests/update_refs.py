"""float64 numpy references for the kernels at the two ends of the DQN and A3C updates -- a helper of
test_update_kernels_host.py (which checks these references on the CPU) and test_update_kernels_gpu.py
(which holds the kernels to them). Not collected by pytest.

  philox4x32_10   vectorised Philox4x32-10 (oracle.native.philox one counter at a time)
  sample_uniforms r48_sample_actions' 24-bit uniform of every row
  huber           per-row smooth-L1 loss (beta 1) and the gradient of its mean
  adam            one torch.optim.Adam step (bias-corrected, eps outside the square root)
  returns         r48_discounted_returns' [T][n] slab, lengths clamped to 0..T
  q_head          the Q head Linear(1024 -> 4) and its backward, with the magnitude sums of the bounds
  bn_forward      training-mode BatchNorm (+ residual, ReLU): statistics, coefficients, output, running
                  statistics (bn_from_sums: the same from given sums), with the bounds' magnitude sums
  bn_backward     its backward from the masked gradient (bn_backward_from_sums: from given sums)
  conv3x3         the 3x3 (pad 1) convolution on the 4x4 grid, channels-last, its data gradient
                  (conv3x3_dgrad) and weight gradient (conv3x3_wgrad), with the bounds' magnitude sums
RMSProp and the TD target are oracle/a3c_ref.py's and oracle/dqn_ref.py's.
"""
import numpy as np

from oracle import a3c_ref as R

U = 2.0 ** -24          # fp32 unit roundoff (round to nearest)
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr uint32-valued [n, 4], key (k0, k1) -> uint32 [n, 4]: ten rounds of Philox4x32."""
    c = [np.asarray(ctr)[:, k].astype(np.uint64) & MASK32 for k in range(4)]
    k0, k1 = np.uint64(int(key[0]) & 0xFFFFFFFF), np.uint64(int(key[1]) & 0xFFFFFFFF)
    m0, m1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    s = np.uint64(32)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                       # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> s) ^ c[1] ^ k0, p1 & MASK32, (p0 >> s) ^ c[3] ^ k1, p0 & MASK32]
        k0 = (k0 + np.uint64(0x9E3779B9)) & MASK32
        k1 = (k1 + np.uint64(0xBB67AE85)) & MASK32
    return np.stack(c, 1).astype(np.uint32)


def sample_uniforms(n, seed, gid0, ctr):
    """u[i] of r48_sample_actions: Philox4x32-10(key = seed, counter = {gid lo, gid hi, ctr, 0xA3C}),
    gid = gid0 + i, u = (w0 >> 8) / 2^24. float64 (exact: 24 bits)."""
    gid = np.arange(n, dtype=np.uint64) + np.uint64(gid0)
    c = np.stack([gid & MASK32, gid >> np.uint64(32), np.full(n, ctr & 0xFFFFFFFF, np.uint64),
                  np.full(n, 0xA3C, np.uint64)], 1)
    w = philox4x32_10(c, (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    return (w[:, 0] >> np.uint32(8)).astype(np.float64) / 16777216.0


def huber(qa, y):
    """qa, y [n] -> (loss per row [n], gradient of the MEAN loss w.r.t. qa [n]), float64."""
    d = np.asarray(qa, np.float64) - np.asarray(y, np.float64)
    ad = np.abs(d)
    return np.where(ad < 1.0, 0.5 * d * d, ad - 0.5), np.clip(d, -1.0, 1.0) / d.size


def adam(p, g, m, v, t, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8):
    """One step with the 1-based step count t -> (p, m, v); float64 in, float64 out."""
    m = b1 * m + (1.0 - b1) * g
    v = b2 * v + (1.0 - b2) * g * g
    c1, c2 = 1.0 - b1 ** t, 1.0 - b2 ** t
    return p - (lr / c1) * m / (np.sqrt(v / c2) + eps), m, v


def returns(rewards, lengths, bootstrap, gamma, drop_last):
    """[T][n] targets: column i is R.target_values over its first clamp(lengths[i], 0, T) rewards,
    0 from there on (a column of length 0 is all zero)."""
    rewards = np.asarray(rewards, np.float64)
    T, n = rewards.shape
    out = np.zeros((T, n))
    for i in range(n):
        L = int(min(max(int(lengths[i]), 0), T))
        if L:
            out[:L, i] = R.target_values(rewards[:L, i], float(bootstrap[i]), gamma, drop_last=drop_last)
    return out


def q_head(h, w, b, dq):
    """h [B, 1024], w [4, 1024], b [4], dq [B, 4], all float64 holding the values the kernels use
    (bf16-valued h, w, b and dq). -> dict of q, dh, dw, db and the sums of magnitudes |.| that the
    fp32 summation bounds are stated over."""
    return {"q": h @ w.T + b, "q_mag": np.abs(h) @ np.abs(w).T,
            "dh": dq @ w, "dh_mag": np.abs(dq) @ np.abs(w),
            "dw": dq.T @ h, "dw_mag": np.abs(dq).T @ np.abs(h),
            "db": dq.sum(0), "db_mag": np.abs(dq).sum(0)}


def bf16_half_ulp(x):
    """Half a bf16 ulp (8 significant bits) in the binade of |x|: 2^(floor(log2 |x|) - 8); the error of
    rounding x to the nearest bf16 is at most this. Between 2^-9 |x| and 2^-8 |x|; 0 at 0."""
    x = np.abs(np.asarray(x, np.float64))
    _, e = np.frexp(x)                                        # x = f 2^e, f in [0.5, 1)
    return np.where(x > 0, np.ldexp(1.0, e - 1 - 8), 0.0)


def _bn_coefs(mean, var, n, gamma, beta, rm, rv, momentum, eps):
    """The finish of a training-mode BatchNorm from a channel's mean and biased variance over n rows:
    invstd, a = gamma invstd, b = beta - mean a, and the running statistics (None without rm). The
    running variance takes the unbiased n / (n - 1) var for n > 1 and var itself for n = 1 (the
    kernels' choice: torch refuses n = 1)."""
    invstd = 1.0 / np.sqrt(var + eps)
    a = gamma * invstd
    out = {"mean": mean, "var": var, "invstd": invstd, "a": a, "b": beta - mean * a, "rm": None, "rv": None}
    if rm is not None:
        unb = var * (n / (n - 1.0)) if n > 1 else var
        out["rm"] = (1.0 - momentum) * rm + momentum * mean
        out["rv"] = (1.0 - momentum) * rv + momentum * unb
    return out


def bn_from_sums(s1, s2, n, x0, gamma, beta, rm, rv, momentum, eps):
    """From s1 = sum (x - x0) and s2 = sum (x - x0)^2 per channel over n rows (x0 = 0: plain sums):
    mean = x0 + s1 / n, var = max(s2 / n - (s1 / n)^2, 0) and _bn_coefs of them, float64."""
    dm = s1 / n
    return _bn_coefs(x0 + dm, np.maximum(s2 / n - dm * dm, 0.0), n, gamma, beta, rm, rv, momentum, eps)


def bn_forward(x, res, gamma, beta, rm, rv, momentum, eps, relu):
    """x [n, C], res [n, C] or None, gamma, beta, rm, rv [C] (rm, rv None together), float64 holding
    the values the kernels see. -> dict: mean, var (biased, two passes), invstd, a, b, z = a x + b
    (+ res), y = relu?(z), rm, rv after the momentum update, and the magnitudes of the bounds:
    s1_mag = sum |x - x0|, s2_mag = sum (x - x0)^2 (x0 = row 0, the kernels' shift) and
    z_mag = |a x| + |b| + |res|."""
    n = x.shape[0]
    mean = x.mean(0)
    out = _bn_coefs(mean, np.square(x - mean).mean(0), n, gamma, beta, rm, rv, momentum, eps)
    z = out["a"] * x + out["b"]
    mag = np.abs(out["a"] * x) + np.abs(out["b"])
    if res is not None:
        z = z + res
        mag += np.abs(res)
    d0 = x - x[0]
    out.update(z=z, y=np.maximum(z, 0.0) if relu else z, z_mag=mag, s1_mag=np.abs(d0).sum(0),
               s2_mag=np.square(d0).sum(0))
    return out


def bn_backward_from_sums(sg, sgx, n, mean, invstd, gamma):
    """From sg = sum g and sgx = sum g (x - mean) per channel: dbeta = sg, dgamma = invstd sgx and the
    coefficients of dx = a g + cc x + d: a = gamma invstd, cc = -a invstd dgamma / n,
    d = -a dbeta / n - cc mean."""
    dgamma = invstd * sgx
    a = gamma * invstd
    cc = -a * invstd * dgamma / n
    return {"dbeta": sg, "dgamma": dgamma, "a": a, "cc": cc, "d": -a * sg / n - cc * mean}


def bn_backward(g, x, mean, invstd, gamma):
    """g [n, C] (the output gradient already through the ReLU mask), x [n, C], mean, invstd, gamma [C],
    float64. -> dict: dbeta, dgamma, a, cc, d (bn_backward_from_sums), dx = a g + cc x + d -- evaluated
    as a (g - dbeta / n - (x - mean) invstd dgamma / n), the same number without the cancellation of
    cc x + d when |mean| >> std -- and the magnitudes g_mag = sum |g|, gx_mag = sum |g| |x - mean|."""
    n = x.shape[0]
    xc = x - mean
    out = bn_backward_from_sums(g.sum(0), (g * xc).sum(0), n, mean, invstd, gamma)
    out.update(dx=out["a"] * (g - out["dbeta"] / n - xc * (invstd * out["dgamma"] / n)),
               g_mag=np.abs(g).sum(0), gx_mag=(np.abs(g) * np.abs(xc)).sum(0))
    return out


def _zeros(like, shape):
    """Float64 zeros of `shape` of the kind of `like`: a numpy array, or a torch tensor on its device."""
    return like.new_zeros(shape) if hasattr(like, "new_zeros") else np.zeros(shape)


def shift_cells(x, dr, dc):
    """x [B, 16, C] (cell = 4 r + c) -> x at cell (r + dr, c + dc) of the same board, 0 outside the grid."""
    B, _, C = x.shape
    g = x.reshape(B, 4, 4, C)
    out = _zeros(x, (B, 4, 4, C))
    r0, r1, c0, c1 = max(0, -dr), min(4, 4 - dr), max(0, -dc), min(4, 4 - dc)
    out[:, r0:r1, c0:c1] = g[:, r0 + dr:r1 + dr, c0 + dc:c1 + dc]
    return out.reshape(B, 16, C)


def conv3x3(x, w, bias=None, add=None):
    """y[b, p, co] = bias[co] + sum over the taps (kr, kc) and ci of w[co, ci, kr, kc] x[b, p + 4 (kr - 1)
    + (kc - 1), ci] for the taps that stay on the 4x4 grid (pad 1) (+ add[b, p, co]). x [B, 16, cin],
    w [cout, cin, 3, 3], bias [cout], add [B, 16, cout], float64: numpy arrays, or torch tensors (on any
    device: the GPU tests evaluate this same function there). -> (y, mag) [B, 16, cout], mag the sum
    of the magnitudes of every term of y (the products, the bias, the add)."""
    B, _, cin = x.shape
    cout = w.shape[0]
    y, mag = _zeros(x, (B * 16, cout)), _zeros(x, (B * 16, cout))
    for t in range(9):
        xs = shift_cells(x, t // 3 - 1, t % 3 - 1).reshape(B * 16, cin)
        wt = w[:, :, t // 3, t % 3]
        y = y + xs @ wt.T
        mag = mag + abs(xs) @ abs(wt).T
    if bias is not None:
        y, mag = y + bias, mag + abs(bias)
    y, mag = y.reshape(B, 16, cout), mag.reshape(B, 16, cout)
    if add is not None:
        y, mag = y + add, mag + abs(add)
    return y, mag


def conv3x3_dgrad(dy, w, add=None):
    """The gradient of conv3x3 with respect to x: dx[b, q, ci] = sum over the taps and co of
    w[co, ci, kr, kc] dy[b, q - 4 (kr - 1) - (kc - 1), co] for the output cells on the grid (+ add
    [b, q, ci]). dy [B, 16, cout] -> (dx, mag) [B, 16, cin]."""
    B, _, cout = dy.shape
    cin = w.shape[1]
    dx, mag = _zeros(dy, (B * 16, cin)), _zeros(dy, (B * 16, cin))
    for t in range(9):
        ds = shift_cells(dy, 1 - t // 3, 1 - t % 3).reshape(B * 16, cout)
        wt = w[:, :, t // 3, t % 3]
        dx = dx + ds @ wt
        mag = mag + abs(ds) @ abs(wt)
    dx, mag = dx.reshape(B, 16, cin), mag.reshape(B, 16, cin)
    if add is not None:
        dx, mag = dx + add, mag + abs(add)
    return dx, mag


def conv3x3_wgrad(dy, x):
    """The gradient of conv3x3 with respect to w: dw[co, ci, kr, kc] = sum over boards and the cells p
    whose tap stays on the grid of dy[b, p, co] x[b, p + 4 (kr - 1) + (kc - 1), ci]. -> (dw, mag)
    [cout, cin, 3, 3]."""
    B, _, cin = x.shape
    cout = dy.shape[2]
    d = dy.reshape(B * 16, cout)
    dw, mag = _zeros(x, (cout, cin, 3, 3)), _zeros(x, (cout, cin, 3, 3))
    for t in range(9):
        xs = shift_cells(x, t // 3 - 1, t % 3 - 1).reshape(B * 16, cin)
        dw[:, :, t // 3, t % 3] = d.T @ xs
        mag[:, :, t // 3, t % 3] = abs(d).T @ abs(xs)
    return dw, mag
