"""Shared helpers of the kernel-level tests of the fused tile operators' packed and segmented forms (tests/test_gpu_tile_pack.py,
tests/test_gpu_tile_split.py): the tests' weights, a launch of stair_tile_mlp_fwd from named fields, the fp64 references and the
layout of the relu' bit words."""
import ctypes as C

import numpy as np
import torch

from stair_amd._lib import lib, check, TileMlpArgs

DEV = 'cuda:0'
H = 512
STORE_FIRST = 0x40000000


def _gen(T, cnt, salt):
    return torch.Generator().manual_seed(1000 * salt + 37 * T + cnt)


_W = {}


def _lin(i):
    """layer i of the tests' MLPs: (weight [512, 512], bias) on the CPU, made once"""
    if i not in _W:
        g = torch.Generator().manual_seed(77 + i)
        _W[i] = (torch.randn(H, H, generator=g) / H ** 0.5, 0.1 * torch.randn(H, generator=g))
    return _W[i]


_P = {}


def _planes(i, transpose=False):
    from stair_amd import ops
    if (i, transpose) not in _P:
        _P[(i, transpose)] = ops.pack_wfrag(_lin(i)[0].to(DEV), transpose=transpose)
    return _P[(i, transpose)]


def d(t):
    return t.to(DEV)


def i32(a):
    return torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)


def _perm(n, k, g):
    return torch.randperm(n, generator=g)[:k].to(torch.int32)


def _close(got, ref, tol, what):
    err = float((got.cpu().double() - ref.double()).abs().max())
    bound = tol * max(1.0, float(ref.abs().max()))
    assert err < bound, (what, err, bound)


def _launch(cnt, T, layers, tail=0, **kw):
    """stair_tile_mlp_fwd from named fields: layers = [(planes, bias or None, act)], everything else a tensor, an address, a list
    (per-layer arrays), a number or None (left out)"""
    from stair_amd import ops
    a = TileMlpArgs()
    for l, (planes, bias, act) in enumerate(layers):
        a.W[l], a.bias[l], a.act[l] = planes.data_ptr(), (bias.data_ptr() if bias is not None else None), act
    a.n_layers, a.tail, a.cnt, a.T, a.H = len(layers), tail, cnt, T, H
    for k, v in kw.items():
        if v is None:
            continue
        if isinstance(v, (list, tuple)):
            arr = getattr(a, k)
            for l, x in enumerate(v):
                if x is not None:
                    arr[l] = x.data_ptr() if isinstance(x, torch.Tensor) else x
        else:
            setattr(a, k, v.data_ptr() if isinstance(v, torch.Tensor) else v)
    check(lib.stair_tile_mlp_fwd(C.byref(a), ops._stream()))


def _fwd_layers(n, last_relu=True):
    return [(_planes(i), d(_lin(i)[1]), 1 if (i + 1 < n or last_relu) else 0) for i in range(n)]


def _mlp_ref(x, n, last_relu=True):
    """fp64: n layers Lin . ReLU of the tests' weights on x [..., 512]; returns every layer's activation"""
    acts, h = [], x.double()
    for i in range(n):
        w, b = _lin(i)
        h = h @ w.double().t() + b.double()
        if i + 1 < n or last_relu:
            h = torch.relu(h)
        acts.append(h)
    return acts


def _chain_ref(dy2, sv):
    """fp64 of the chain dX = ((dY * relu'(h2)) W2 * relu'(h1)) W1 with the relu' masks of the forward launch's saves"""
    m1, m2 = (sv[0].cpu() > 0).double(), (sv[1].cpu() > 0).double()
    dz2 = dy2.double() * m2
    dz1 = (dz2 @ _lin(1)[0].double()) * m1
    return dz2, dz1, dz1 @ _lin(0)[0].double()


def _fwd2(T, cnt, g, lens=None, drop=None):
    """the forward launch the chain tests build on: 2 layers Lin . ReLU with saves and save_bits, no tail (packing and segments
    as set; bit words for one tile per instance and 64-row segment, the most a launch writes)"""
    x = torch.randn(cnt, T, H, generator=g)
    sv = [torch.zeros(cnt, T, H, device=DEV) for _ in range(2)]
    bits = [torch.zeros(cnt * ((T + 63) // 64), H, dtype=torch.int64, device=DEV) for _ in range(2)]
    kw = dict(X=d(x), x_gstride=T * H, save=sv, save_bits=bits, len=i32(lens) if lens else None)
    if drop:
        kw.update(drop_site=[1, 2], drop_p=drop[0], drop_seed=drop[1])
    _launch(cnt, T, _fwd_layers(2), **kw)
    return x, sv, bits


def _tile_words(rows):
    """rows [tiles, 64, 512] bool -> the tiles' save_bits words [tiles, 512] int64: word 64 w + c, byte j, bit e <-> row w + 8 j of
    the tile, column 8 c + e (bit 63 wraps to the sign, as stored)"""
    tiles = rows.shape[0]
    r = rows.reshape(tiles, 8, 8, 64, 8).long()         # (tile, j, w, c, e)
    sh = 8 * torch.arange(8).reshape(1, 8, 1, 1, 1) + torch.arange(8).reshape(1, 1, 1, 1, 8)
    return (r << sh).sum(dim=(1, 4)).reshape(tiles, H)


def _work_items():
    n = C.c_int64(0)
    assert lib.stair_tile_work_items(C.byref(n), 1) == 0
    return n.value
