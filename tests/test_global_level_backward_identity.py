"""The identities the one-launch backward of the global level rests on (csrc/global_level_bwd.hip), in fp64 torch on the CPU:
FP3 interpolates with k = 1 and weight 1 from the plot's one source, so the input gradient and the weight gradient of its
interpolated part collapse to per-plot sums; the BatchNorm sums of SA3 over its sparse output gradient are B-term sums; and the
BatchNorm sums of FP3 taken directly over the rows equal what the consumer identity (sn2_fp_bn_sums) derives from FP2's dW, db."""
import torch

F64 = torch.float64


def test_interpolated_part_of_fp3_collapses_to_per_plot_sums():
    g = torch.Generator().manual_seed(1)
    B, M2 = 3, 37
    dp = torch.randn(B, M2, 64, generator=g, dtype=F64)
    Wa = torch.randn(64, 64, generator=g, dtype=F64)            # W[:, 0:64]
    x3 = torch.randn(B, 64, generator=g, dtype=F64)
    per_row = (dp @ Wa).sum(1)                                   # sum_rows (dp . W_a)
    per_plot = dp.sum(1) @ Wa                                    # (sum_rows dp) . W_a
    assert torch.allclose(per_row, per_plot, rtol=1e-12, atol=1e-12)
    u = x3[:, None, :].expand(B, M2, 64)                         # every row's interpolated input is the plot feature
    dW_rows = torch.einsum("bro,brk->ok", dp, u)
    dW_plots = torch.einsum("bo,bk->ok", dp.sum(1), x3)
    assert torch.allclose(dW_rows, dW_plots, rtol=1e-12, atol=1e-12)


def test_batchnorm_sums_of_sa3_over_the_sparse_gradient_are_b_term_sums():
    g = torch.Generator().manual_seed(2)
    B, M2 = 4, 29
    h = torch.relu(torch.randn(B, M2, 64, generator=g, dtype=F64))
    mean, invstd = h.mean((0, 1)), 1.0 / torch.sqrt(h.var((0, 1), unbiased=False) + 1e-5)
    arg = torch.randint(0, M2, (B, 64), generator=g)
    dx3 = torch.randn(B, 64, generator=g, dtype=F64)
    dx3[1, 7] = 0.0
    dy = torch.zeros(B, M2, 64, dtype=F64)
    dy.scatter_(1, arg[:, None, :], dx3[:, None, :])
    xhat = (h - mean) * invstd
    dbeta, dgamma = dy.sum((0, 1)), (dy * xhat).sum((0, 1))
    xh_arg = xhat.gather(1, arg[:, None, :])[:, 0, :]
    assert torch.allclose(dbeta, dx3.sum(0), rtol=1e-12, atol=1e-12)
    assert torch.allclose(dgamma, (dx3 * xh_arg).sum(0), rtol=1e-12, atol=1e-12)


def test_direct_batchnorm_sums_of_fp3_equal_the_consumer_identity():
    """FP2 reads y = a h + c of FP3 through a linear interpolation T: u = T y.  With G = T^T (dp2 W_A) the gradient of y,
    sum G = d beta and sum G xhat = d gamma; the consumer identity gets the same two sums from FP2's dW_A = dp2^T u and db = sum dp2
    only where T's rows sum to one and y is affine in xhat: dW_A = dp2^T T (gamma xhat + beta)."""
    g = torch.Generator().manual_seed(3)
    R1, R2, C, CO = 50, 20, 64, 34
    xhat = torch.randn(R2, C, generator=g, dtype=F64)
    gamma, beta = torch.rand(C, generator=g, dtype=F64) + 0.5, torch.randn(C, generator=g, dtype=F64)
    T = torch.rand(R1, R2, generator=g, dtype=F64)
    T = T / T.sum(1, keepdim=True)
    dp2 = torch.randn(R1, CO, generator=g, dtype=F64)
    Wa = torch.randn(CO, C, generator=g, dtype=F64)
    G = T.t() @ (dp2 @ Wa)                                       # the gathered gradient of FP3's output
    direct_beta, direct_gamma = G.sum(0), (G * xhat).sum(0)
    dWa = dp2.t() @ (T @ (gamma * xhat + beta))                  # FP2's own weight gradient of the interpolated columns
    db = dp2.sum(0)
    ident_beta = db @ Wa                                         # sum_o db[o] W[o, c]
    ident_gamma = ((Wa * dWa).sum(0) - beta * ident_beta) / gamma
    assert torch.allclose(direct_beta, ident_beta, rtol=1e-10, atol=1e-10)
    assert torch.allclose(direct_gamma, ident_gamma, rtol=1e-10, atol=1e-10)
