"""Plain-torch restatement of the LocalTransformer of ACTRv2 (CP/det3d/models/model_utils/pointformer.py:10-44, 250-380),
the yardstick of the training tests: every step written out on tensors of whatever dtype the caller hands in (float64 =
the reference, float32 on the host = what plain fp32 arithmetic makes of the same formula).  Nothing here calls the
product's modules or kernels: grouping is an index gather, the attention is softmax(q k^T / sqrt(head_dim)) v, LayerNorm
and BatchNorm are their defining formulas, the 'unique' write-back keeps the LOWEST flat (centre, sample) position of a
point (pointformer.py:320-328).  Geometry (group indices / grouped coordinates) is an input.

Test infrastructure only; tests/test_lt_train_host.py checks it against the reference's golden output and against
torch.autograd on the product's layer."""
import math

import numpy as np
import torch


def attention(qkv, tokens, groups, heads):
    """qkv [tokens * groups, 3 * C] rows (row = token * groups + group; q | k | v) -> [tokens * groups, C]."""
    C = qkv.shape[1] // 3
    D = C // heads
    q, k, v = [t.reshape(tokens, groups, heads, D).permute(1, 2, 0, 3) for t in qkv.split(C, 1)]       # [G, H, L, D]
    p = torch.softmax(q @ k.transpose(-1, -2) / math.sqrt(D), -1)
    return (p @ v).permute(2, 0, 1, 3).reshape(tokens * groups, C)


def layer_norm(x, weight, bias, eps=1e-5):
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + eps) * weight + bias


def encoder_layer(p, x, heads, prefix=""):
    """The pre-norm layer of the reference (pointformer.py:34-43): x = LN1(x); x = x + MHA(x); x = LN2(x); x = x + FFN(x):
    both residuals start from the NORMALISED tensor.  p: name -> tensor; x [tokens, groups, C]."""
    L, G, C = x.shape
    P = lambda k: p[prefix + k]                                                               # noqa: E731
    x1 = layer_norm(x.reshape(L * G, C), P("norm1.weight"), P("norm1.bias"))
    qkv = x1 @ P("self_attn.in_proj_weight").t() + P("self_attn.in_proj_bias")
    a = attention(qkv, L, G, heads) @ P("self_attn.out_proj.weight").t() + P("self_attn.out_proj.bias")
    x3 = layer_norm(x1 + a, P("norm2.weight"), P("norm2.bias"))
    f = torch.relu(x3 @ P("linear1.weight").t() + P("linear1.bias")) @ P("linear2.weight").t() + P("linear2.bias")
    return (x3 + f).view(L, G, C)


def winners(group_idx_b, n_points):
    """Per point the flat (centre * nsample + sample) position the 'unique' scatter keeps, -1 where it is in no group:
    written back to front, so that the LOWEST position is the last write."""
    flat = np.asarray(group_idx_b).reshape(-1)
    win = np.full((n_points,), -1, np.int64)
    win[flat[::-1]] = np.arange(len(flat) - 1, -1, -1)
    return win


def local_transformer(p, group_idx, group_xyz, rows, heads, num_layers, bn_training, stats=None, eps=1e-5):
    """p: name -> tensor of a LocalTransformer (`pe.0.conv.weight`, `pe.0.bn.*`, `pe.1.conv.*`, `chunk.layers.j.*`);
    group_idx [B, np, ns] integer; group_xyz [B, 3, np, ns] (absolute coordinates); rows [B, N, C] -> [B, N, C].
    bn_training: BatchNorm on the statistics of the batch (biased variance), else on the running statistics; `stats`
    (a dict) receives the batch mean and the UNBIASED variance, what the running statistics move towards."""
    B, N, C = rows.shape
    gi = torch.as_tensor(np.asarray(group_idx), dtype=torch.long)
    _, np_, ns = gi.shape
    grouped = torch.gather(rows, 1, gi.reshape(B, -1, 1).expand(B, np_ * ns, C)).view(B, np_, ns, C)
    h = group_xyz.permute(0, 2, 3, 1) @ p["pe.0.conv.weight"][:, :, 0, 0].t()                # [B, np, ns, C/2]
    if "pe.0.conv.bias" in p:
        h = h + p["pe.0.conv.bias"]
    if "pe.0.bn.weight" in p:
        if bn_training:
            mean = h.mean((0, 1, 2))
            var = ((h - mean) ** 2).mean((0, 1, 2))
            if stats is not None:
                n = h.numel() // h.shape[-1]
                stats["mean"], stats["var_unbiased"] = mean.detach(), var.detach() * n / (n - 1)
        else:
            mean, var = p["pe.0.bn.running_mean"], p["pe.0.bn.running_var"]
        h = (h - mean) / torch.sqrt(var + eps) * p["pe.0.bn.weight"] + p["pe.0.bn.bias"]
    pe = torch.relu(h) @ p["pe.1.conv.weight"][:, :, 0, 0].t() + p["pe.1.conv.bias"]
    x = (grouped + pe).permute(2, 0, 1, 3).reshape(ns, B * np_, C)                           # [ns, B * np, C]
    for j in range(num_layers):
        x = encoder_layer(p, x, heads, "chunk.layers.%d." % j)
    y = x.view(ns, B, np_, C).permute(1, 2, 0, 3).reshape(B, np_ * ns, C)                    # flat position = centre * ns + sample
    out = []
    for b in range(B):
        win = torch.from_numpy(winners(gi[b].numpy(), N))
        out.append(torch.where((win >= 0)[:, None], y[b][win.clamp(min=0)], rows[b]))
    return torch.stack(out)


def module_tensors(module):
    """name -> parameter / buffer of a module (the tensors themselves: gradients land on the module's parameters)."""
    d = dict(module.named_parameters())
    d.update(dict(module.named_buffers()))
    return d


def errors(got, want, plain32):
    """(max |got - want| / max |want|, the same for the plain fp32 host evaluation, L2-relative error of `got`)."""
    want = want.detach().double()
    scale = float(want.abs().max())
    g = got.detach().double().cpu()
    return (float((g - want).abs().max()) / scale, float((plain32.detach().double() - want).abs().max()) / scale,
            float((g - want).norm() / want.norm()))
