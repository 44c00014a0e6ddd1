"""Every module of dualfusion/spconv as a dense float64 network, written from torch.nn.functional alone (CPU).

A sparse tensor is densified to [B, C, *shape] with zeros at the inactive cells, the layer is the dense convolution of the
same geometry, and the result is read back at the layer's active output set.  Nothing here knows a rulebook, a neighbour
table, a kernel-offset order or the `view(K, cin, cout)` of the filters: the weight goes to torch as a permutation of the
module's own [*kernel, Cin, Cout] tensor, never flipped.

    forward / SubM   F.convNd(X, w.permute(Cout, Cin, *kernel), stride, padding)            out[o] = sum_t x[o st - p + t] w[t]
    transposed       F.conv_transposeNd(X, w.permute(Cin, Cout, *kernel), stride, padding, output_padding, dilation)
                                                                                            out[i st - p + t d] += x[i] w[t]
    inverse          the transposed form with the forward convolution's stride / padding and the output_padding that restores
                     the forward convolution's input shape, read at that convolution's input sites
    pool             F.max_poolNd(X.clamp_min(0)): the pooled value starts from zero

The active output set of a layer is `conv(mask, ones) > 0` with the same geometry (SubM, inverse: the given sites).  The
output size of a transposed layer is (s - 1) st - 2 p + k + output_padding in the modules -- the dilation does not enter --, so
torch's larger result is cropped to it.  Bias is added at active sites only.

Every function takes (rows float64 [N, C], indices [N, 1 + ndim] (b, *cell), spatial shape, batch, weight, bias, geometry...)
for ndim = 2 or 3 alike and returns (active output coordinates int64 [n_out, 1 + ndim], output spatial shape, output rows
[n_out, Cout]), differentiable by torch autograd.  Strided and transposed outputs come in ascending (b, *cell) order, SubM /
inverse outputs in the order of the given sites; `rows_at` maps them onto any other row order by coordinate.

`abs_bound` is the same computation on |x|, |w|, |bias| (and |g| for the gradients): the elementwise magnitude A against
which a rounding bound is stated (`bound`)."""
import numpy as np
import torch
import torch.nn.functional as F

F64 = torch.float64
_CONV = {2: F.conv2d, 3: F.conv3d}
_CONVT = {2: F.conv_transpose2d, 3: F.conv_transpose3d}
_POOL = {2: F.max_pool2d, 3: F.max_pool3d}

MODES = ("fp32", "split", "split3", "bf16")
FP32_GRADE = 1e-4          # max |got - ref| <= FP32_GRADE max |ref|: what test_conv_backward_golden_and_autograd holds the modules to
BF16_UNIT = 2.0 ** -8      # unit roundoff of a value rounded to 8 significant bits
BF16_ACCUM = 2e-5          # fp32 accumulation (PROD of tests/test_gpu_bf16train.py), of the largest magnitude


def _t(a, dtype):
    if isinstance(a, torch.Tensor):
        return a.detach().cpu().to(dtype)
    return torch.tensor(np.asarray(a), dtype=dtype)            # (a copy: shared reference arrays are read-only)


def _lst(v, ndim):
    return [int(e) for e in v] if isinstance(v, (list, tuple)) else [int(v)] * ndim


def _where(indices):
    idx = _t(indices, torch.int64)
    return (idx[:, 0], slice(None)) + tuple(idx[:, 1 + d] for d in range(idx.shape[1] - 1))


def densify(rows, indices, shape, batch):
    """rows [N, C] at indices [N, 1 + ndim] -> [batch, C, *shape] float64, zero elsewhere (differentiable in rows)."""
    idx = _t(indices, torch.int64)
    cl = torch.zeros((batch,) + tuple(shape) + (rows.shape[1],), dtype=rows.dtype)
    cl = cl.index_put(tuple(idx[:, d] for d in range(idx.shape[1])), rows)
    return cl.movedim(-1, 1)


def gather(dense, coords):
    """[B, C, *shape] -> the rows [n, C] at coords [n, 1 + ndim]"""
    return dense[_where(coords)]


def mask_of(indices, shape, batch):
    return densify(torch.ones((len(indices), 1), dtype=F64), indices, shape, batch)


def coords_of(mask):
    """the cells of a [B, 1, *shape] mask that are > 0, in ascending (b, *cell) order"""
    return torch.nonzero(mask[:, 0] > 0)


def occupancy(indices, shape, batch, kernel, stride, padding, transposed=False, output_padding=0, dilation=1):
    """The active output set of a strided or transposed layer: conv(mask, ones) > 0 -> (coords, out_shape)."""
    ndim = len(shape)
    ones = torch.ones((1, 1) + tuple(_lst(kernel, ndim)), dtype=F64)
    m = _dense_conv(mask_of(indices, shape, batch), ones, shape, stride, padding, transposed, output_padding, dilation)
    return coords_of(m), list(m.shape[2:])


def _dense_conv(X, wt, shape, stride, padding, transposed, output_padding=0, dilation=1):
    """wt in torch's layout.  Transposed: cropped to the modules' output size (see the module docstring)."""
    ndim = len(shape)
    stride, padding, dilation = _lst(stride, ndim), _lst(padding, ndim), _lst(dilation, ndim)
    if not transposed:
        return _CONV[ndim](X, wt, None, stride, padding, dilation)
    op, ks = _lst(output_padding, ndim), list(wt.shape[2:])
    Y = _CONVT[ndim](X, wt, None, stride, padding, op, 1, dilation)
    size = [(shape[d] - 1) * stride[d] - 2 * padding[d] + ks[d] + op[d] for d in range(ndim)]
    assert all(Y.shape[2 + d] - size[d] == (dilation[d] - 1) * (ks[d] - 1) for d in range(ndim))
    return Y[(slice(None), slice(None)) + tuple(slice(0, s) for s in size)]


def _rows_out(Y, coords, bias):
    out = gather(Y, coords)
    return out if bias is None else out + bias


def _perm(weight, transposed):
    """the module's [*kernel, Cin, Cout] as torch's [Cout, Cin, *kernel] (transposed: [Cin, Cout, *kernel])"""
    nd = weight.dim() - 2
    return weight.permute(*((nd, nd + 1) if transposed else (nd + 1, nd)), *range(nd))


def conv(rows, indices, shape, batch, weight, bias=None, stride=1, padding=0):
    """SparseConv2d / SparseConv3d"""
    ks = list(weight.shape[:-2])
    coords, out_shape = occupancy(indices, shape, batch, ks, stride, padding)
    Y = _dense_conv(densify(rows, indices, shape, batch), _perm(weight, False), shape, stride, padding, False)
    return coords, out_shape, _rows_out(Y, coords, bias)


def subm(rows, indices, shape, batch, weight, bias=None):
    """SubMConv2d / SubMConv3d (odd kernels): padding k // 2, stride 1, read at the input sites in their order."""
    ks = list(weight.shape[:-2])
    assert all(k % 2 == 1 for k in ks)
    Y = _dense_conv(densify(rows, indices, shape, batch), _perm(weight, False), shape, 1, [k // 2 for k in ks], False)
    coords = _t(indices, torch.int64)
    return coords, list(shape), _rows_out(Y, coords, bias)


def conv_transpose(rows, indices, shape, batch, weight, bias=None, stride=1, padding=0, output_padding=0, dilation=1):
    """SparseConvTranspose2d / SparseConvTranspose3d"""
    ks = list(weight.shape[:-2])
    coords, out_shape = occupancy(indices, shape, batch, ks, stride, padding, True, output_padding, dilation)
    Y = _dense_conv(densify(rows, indices, shape, batch), _perm(weight, True), shape, stride, padding, True, output_padding,
                    dilation)
    return coords, out_shape, _rows_out(Y, coords, bias)


def inverse(rows, indices, shape, batch, weight, bias=None, sites=None, sites_shape=None, stride=1, padding=0):
    """SparseInverseConv3d behind a forward convolution (kernel of `weight`, stride, padding) that took `sites` on
    `sites_shape` to `indices` on `shape`: every pair (i, o) of tap t of that convolution adds rows[o] . weight[t] to out[i]."""
    ndim = len(shape)
    ks, stride, padding = list(weight.shape[:-2]), _lst(stride, ndim), _lst(padding, ndim)
    op = [sites_shape[d] - ((shape[d] - 1) * stride[d] - 2 * padding[d] + ks[d]) for d in range(ndim)]
    assert all(0 <= o < s for o, s in zip(op, stride)), "not the output of that convolution"
    Y = _dense_conv(densify(rows, indices, shape, batch), _perm(weight, True), shape, stride, padding, True, op)
    assert list(Y.shape[2:]) == list(sites_shape)
    coords = _t(sites, torch.int64)
    return coords, list(sites_shape), _rows_out(Y, coords, bias)


def maxpool(rows, indices, shape, batch, kernel, stride=1, padding=0):
    """SparseMaxPool2d / SparseMaxPool3d: max(0, the active inputs of the window)"""
    ndim = len(shape)
    coords, out_shape = occupancy(indices, shape, batch, kernel, stride, padding)
    Y = _POOL[ndim](densify(rows, indices, shape, batch).clamp_min(0), _lst(kernel, ndim), _lst(stride, ndim), _lst(padding, ndim))
    assert list(Y.shape[2:]) == out_shape
    return coords, out_shape, gather(Y, coords)


def dense(rows, indices, shape, batch):
    """SparseConvTensor.dense(): [B, C, *shape]"""
    return densify(rows, indices, shape, batch)


# ---------------------------------------------------------------------------------------------------- rows by coordinate
def flat_key(coords, shape):
    c = _t(coords, torch.int64)
    key = c[:, 0]
    for d, s in enumerate(shape):
        key = key * int(s) + c[:, 1 + d]
    return key


def has_duplicates(coords, shape):
    key = flat_key(coords, shape)
    return len(torch.unique(key)) != len(key)


def same_set(a, b, shape):
    ka, kb = torch.sort(flat_key(a, shape))[0], torch.sort(flat_key(b, shape))[0]
    return ka.shape == kb.shape and bool((ka == kb).all())


def rows_at(ref_coords, shape, coords):
    """-> index i with ref_coords[i] == coords (both duplicate-free, the same set): ref_rows[i] are the rows in the order of
    `coords`."""
    kr, kc = flat_key(ref_coords, shape), flat_key(coords, shape)
    order = torch.argsort(kr)
    pos = order[torch.searchsorted(kr[order], kc)]
    assert bool((kr[pos] == kc).all())
    return pos


# -------------------------------------------------------------------------------------------------------------- bounds
def abs_bound(fn, rows, indices, shape, batch, weight=None, bias=None, grad=None, **geometry):
    """`fn` (one of the functions above, or any network built from them with the same signature) on |rows|, |weight|, |bias|:
    -> A_out, or with grad (the rows of d loss / d out, in the order of fn's output) -> (A_out, A of d rows, A of d weight,
    A of d bias or None): the same backward on |grad|."""
    x = rows.detach().abs().requires_grad_(True)
    w = weight.detach().abs().requires_grad_(True)
    b = bias.detach().abs().requires_grad_(True) if bias is not None else None
    out = fn(x, indices, shape, batch, w, b, **geometry)[2]
    if grad is None:
        return out.detach()
    gs = torch.autograd.grad(out, [x, w] + ([b] if b is not None else []), grad_outputs=grad.detach().abs())
    return out.detach(), gs[0], gs[1], (gs[2] if b is not None else None)


def bf16_factor(layers=1):
    """Two operands of every product rounded to 8 significant bits, `layers` products in a row: (1 + 2^-8)^(2 layers) - 1;
    one layer: 2^-7 (1 + 2^-9)."""
    return (1.0 + BF16_UNIT) ** (2 * layers) - 1.0


def excess(got, ref, A=None, mode="fp32", layers=1):
    """-> (max |got - ref| / max |ref|, the largest |got - ref| / bound): within the bound when the second is <= 1.
    "bf16": elementwise bf16_factor(layers) A + layers 2e-5 max A; every other mode (and layers that have none): 1e-4 max |ref|."""
    got, ref = got.detach().cpu().to(F64), ref.detach().to(F64)
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    if ref.numel() == 0:
        return 0.0, 0.0
    d = (got - ref).abs()
    top = max(float(ref.abs().max()), 1e-300)
    if mode == "bf16":
        limit = bf16_factor(layers) * A + layers * BF16_ACCUM * float(A.max())
        return float(d.max()) / top, float((d / limit).max())
    return float(d.max()) / top, float(d.max()) / (FP32_GRADE * top)
