"""A float64 reference of the fused sparse-convolution layer, in plain torch (index-select, matmul, index-add) and without a
call into the package under test: what tests/test_gpu_conv_configs.py compares every launch configuration of the matrix-core
kernels with.  Runs wherever its tensors live (the large cases keep them on the device, in float64).

    out[o, g*cout + c] = relu?( (sum_k sum_ci x[nbr[k, o], g*stride + ci] * filt[g, k, ci, c] + bias) * scale + shift + residual )

with nbr[k, o] = -1 for "no neighbour at offset k" -- a row without any neighbour is the epilogue of zero.
tests/test_conv_reference_host.py checks it against the numpy loop of test_sparse_conv_split_precision and shows that one
moved neighbour index or one swapped filter tap is far above every bound it is used with."""
import torch


def conv_acc_f64(x, filt, nbr, n_out, groups=1, in_group_stride=0):
    """The contraction alone -> float64 [n_out, groups * cout].  x [n_in, channels], filt [K, cin, cout] (one group) or
    [groups, K, cin, cout], nbr int [K, n_out]; group g reads the input columns g * in_group_stride .. + cin."""
    x = x.double()
    filt = filt.double()
    if filt.dim() == 3:
        filt = filt[None]
    assert filt.shape[0] == groups and nbr.shape[1] == n_out and nbr.shape[0] == filt.shape[1]
    K, cin, cout = filt.shape[1:]
    acc = torch.zeros((n_out, groups * cout), dtype=torch.float64, device=x.device)
    for k in range(K):
        rows = (nbr[k] >= 0).nonzero(as_tuple=True)[0]
        if rows.numel() == 0:
            continue
        src = x.index_select(0, nbr[k].index_select(0, rows).long())
        for g in range(groups):
            c0 = g * in_group_stride
            acc[:, g * cout:(g + 1) * cout].index_add_(0, rows, src[:, c0:c0 + cin] @ filt[g, k])
    return acc


def epilogue_f64(acc, bias=None, scale=None, shift=None, residual=None, relu=False):
    """The fused epilogue on a float64 contraction, in the kernels' order: + bias, * scale, + shift, + residual, ReLU."""
    y = acc.clone()
    if bias is not None:
        y = y + bias.double()
    if scale is not None:
        y = y * scale.double()
    if shift is not None:
        y = y + shift.double()
    if residual is not None:
        y = y + residual.double()
    return y.clamp_min(0) if relu else y


def conv_rows_f64(x, filt, nbr, n_out, bias=None, scale=None, shift=None, residual=None, relu=False, groups=1,
                  in_group_stride=0):
    """The fused layer -> float64 [n_out, groups * cout]."""
    return epilogue_f64(conv_acc_f64(x, filt, nbr, n_out, groups, in_group_stride), bias, scale, shift, residual, relu)
