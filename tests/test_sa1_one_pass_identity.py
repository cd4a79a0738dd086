"""The algebra behind the one-pass SA1 backward (csrc/sa_mfma.hip, "ONE-PASS ROUTE"), on the CPU in fp64.

For a two-block local MLP (Linear -> ReLU -> BatchNorm(train)) x 2 followed by a scatter-max over the centroids, the first
block's weight gradient is LINEAR in (dgamma0, dbeta0):

    [dW0 | db0] = diag(gamma0 s0) (S_g - diag(dgamma0 / E) S_x - diag(dbeta0 / E) S_m)
    S_g = sum_e (m g)_e (x) in_e,   S_x = sum_e (m xhat)_e (x) in_e,   S_m = sum_e m_e (x) in_e

with m = [h > 0], xhat = (h - mean0) s0, g = d loss / d (BatchNorm output of block 0), in_e = [input_e | 1] -- so the three sums
can be taken in the same pass over the messages that sums dgamma0, dbeta0.  Yardstick: torch autograd in fp64, agreement to
1e-12 of the tensor's magnitude; a channel that is never active must come out exactly zero."""
import torch

E, M, CIN, C1, C2 = 3000, 120, 11, 16, 16
EPS = 1e-5
ALWAYS, NEVER = 3, 7


def _bn(h, gamma, beta):
    mu = h.mean(0)
    s = 1.0 / torch.sqrt(h.var(0, unbiased=False) + EPS)
    xhat = (h - mu) * s
    return gamma * xhat + beta, xhat, s


def test_first_block_gradient_from_three_sums_matches_autograd_fp64():
    g = torch.Generator().manual_seed(11)
    f64 = torch.float64
    x = torch.randn(E, CIN, generator=g, dtype=f64)
    cen = torch.randint(0, M, (E,), generator=g)
    W0 = (torch.randn(C1, CIN, generator=g, dtype=f64) * 0.4).requires_grad_(True)
    b0 = torch.randn(C1, generator=g, dtype=f64) * 0.2
    b0[ALWAYS], b0[NEVER] = 60.0, -60.0
    b0.requires_grad_(True)
    gamma0 = (torch.rand(C1, generator=g, dtype=f64) + 0.5).requires_grad_(True)
    beta0 = (torch.randn(C1, generator=g, dtype=f64) * 0.1).requires_grad_(True)
    W1 = (torch.randn(C2, C1, generator=g, dtype=f64) * 0.3).requires_grad_(True)
    b1 = (torch.randn(C2, generator=g, dtype=f64) * 0.1).requires_grad_(True)
    gamma1 = torch.rand(C2, generator=g, dtype=f64) + 0.5
    gamma1[::3] *= -1.0                                   # negative scales: the maximum of the output is the minimum of h
    gamma1.requires_grad_(True)
    beta1 = (torch.randn(C2, generator=g, dtype=f64) * 0.1).requires_grad_(True)
    dout = torch.randn(M, C2, generator=g, dtype=f64)

    h = torch.relu(x @ W0.t() + b0)
    assert bool((h[:, ALWAYS] > 0).all()) and bool((h[:, NEVER] == 0).all())
    y1, xhat, s0 = _bn(h, gamma0, beta0)
    y1.retain_grad()
    y2, _, _ = _bn(torch.relu(y1 @ W1.t() + b1), gamma1, beta1)
    # scatter-max with an explicit winner per (centroid, channel): the gradient goes to that one message
    out = torch.zeros(M, C2, dtype=f64)
    for c in range(M):
        idx = (cen == c).nonzero()[:, 0]
        if idx.numel():
            win = idx[y2[idx].argmax(0)]
            out[c] = y2[win, torch.arange(C2)]
    (out * dout).sum().backward()

    with torch.no_grad():
        gy = y1.grad                                      # g
        m = (h > 0).to(f64)
        inp = torch.cat([x, torch.ones(E, 1, dtype=f64)], 1)
        dgamma0, dbeta0 = (gy * xhat).sum(0), gy.sum(0)
        S_g, S_x, S_m = (m * gy).t() @ inp, (m * xhat).t() @ inp, m.t() @ inp
        got = (gamma0 * s0)[:, None] * (S_g - (dgamma0 / E)[:, None] * S_x - (dbeta0 / E)[:, None] * S_m)
        want = torch.cat([W0.grad, b0.grad[:, None]], 1)
        # the sums pass C already takes are the BatchNorm gradients themselves
        assert float((dgamma0 - gamma0.grad).abs().max()) <= 1e-12 * float(gamma0.grad.abs().max())
        assert float((dbeta0 - beta0.grad).abs().max()) <= 1e-12 * float(beta0.grad.abs().max())
        err = float((got - want).abs().max()) / float(want.abs().max())
        print(f"one-pass form vs autograd (fp64): {err:.2e} of the tensor's magnitude")
        assert err <= 1e-12
        assert float(want[ALWAYS].abs().max()) > 0
        assert bool((got[NEVER] == 0).all()) and bool((want[NEVER] == 0).all())
