"""The backward halves of the exported building-block families (include/stair_hip.h: stair_cosine_attn_bwd,
stair_temporal_relate_bwd) against torch autograd of the oracle's restatement of the same operators
(oracle/nmn_oracle.py: cos_rows / op_existsframe for modules.py:162-217, temporal_relate for modules.py:255-277,317-323)."""
import numpy as np
import pytest
import torch

from helpers import oracle_weights
from oracle import nmn_oracle as O
from stair_amd import spec

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


@pytest.mark.parametrize('G,T,H,npairs', [(3, 8, 64, 5), (4, 64, 512, 9), (1, 33, 128, 1), (3, 33, 192, 5), (2, 40, 320, 4)])
def test_cosine_attn_backward_matches_autograd(G, T, H, npairs):
    from stair_amd import ops
    g = torch.Generator().manual_seed(G + T + H)
    F = torch.randn(G, T, H, generator=g, dtype=torch.float64, requires_grad=True)
    K = torch.randn(npairs + 2, H, generator=g, dtype=torch.float64, requires_grad=True)
    f_idx = torch.randint(0, G, (npairs,), generator=g, dtype=torch.int32)
    k_idx = torch.randint(0, npairs + 2, (npairs,), generator=g, dtype=torch.int32)       # repeats: tiles and rows are shared by pairs
    d_att = torch.randn(npairs, T, generator=g, dtype=torch.float64)
    att = torch.stack([O.op_existsframe(K[int(k_idx[p])], F[int(f_idx[p])]).reshape(T) for p in range(npairs)])
    (att * d_att).sum().backward()
    d = lambda t: t.detach().float().to(DEV)
    got = ops.cosine_attn(d(F), f_idx.to(DEV), d(K), k_idx.to(DEV), npairs, T, H)
    assert float((got.cpu().double() - att.detach()).abs().max()) < 1e-5
    dF, dK = ops.cosine_attn_bwd(d(F), f_idx.to(DEV), d(K), k_idx.to(DEV), d(d_att), npairs, T, H)
    for a, ref in ((dF, F.grad), (dK, K.grad)):
        scale = max(1.0, float(ref.abs().max()))
        assert float((a.cpu().double() - ref).abs().max()) < 2e-5 * scale


@pytest.mark.parametrize('mode', ['while', 'before', 'after', 'between'])
@pytest.mark.parametrize('T,conv', [(64, True), (24, True), (8, False)])
def test_temporal_relate_backward_matches_autograd(mode, T, conv):
    from stair_amd import ops
    config = dict(spec.DEFAULT_CONFIG, hidden_size=64, video_size=128, max_video_length=T if not conv else 64)
    w = {k: (v.double().requires_grad_(True) if 'Temporal.relate' in k else v) for k, v in oracle_weights(config, seed=3).items()}
    assert (w['submodules.Temporal.relate.before.0.weight'].dim() == 3) == conv
    g = torch.Generator().manual_seed(T)
    n, Ks = 5, [1, 2, 1, 2, 2]
    rows = sum(Ks)
    att = torch.rand(rows, T, generator=g, dtype=torch.float64, requires_grad=True)
    d_out = torch.randn(n, T, generator=g, dtype=torch.float64)
    starts = np.concatenate([[0], np.cumsum(Ks)])[:-1]
    outs = [O.temporal_relate(w, mode, att[int(starts[i]): int(starts[i]) + Ks[i]].mean(dim=0)) for i in range(n)]
    (torch.stack(outs) * d_out).sum().backward()
    modes = {'while': 0, 'before': 1, 'after': 2, 'between': 3}
    names = ['submodules.Temporal.relate.%s.%d.%s' % (mode, l, p) for l in (0, 2, 4) for p in ('weight', 'bias')] if mode != 'while' else None
    w6 = [w[nm].detach().float().reshape(-1 if conv and nm.endswith('weight') else w[nm].shape).contiguous().to(DEV) for nm in names] if names else [None] * 6
    d = lambda t: t.detach().float().to(DEV)
    att_idx = torch.tensor(starts, dtype=torch.int32, device=DEV)
    att_k = torch.tensor(Ks, dtype=torch.int32, device=DEV)
    ksize = int(w['submodules.Temporal.relate.before.0.weight'].numel()) if conv else 0
    got = ops.temporal_relate(d(att), att_idx, att_k, n, T, modes[mode], conv, ksize, w6)
    assert float((got.cpu().double() - torch.stack(outs).detach()).abs().max()) < 1e-5
    d_att, dws = ops.temporal_relate_bwd(d(att), att_idx, att_k, d(d_out), n, T, modes[mode], conv, ksize, w6)
    assert float((d_att.cpu().double() - att.grad).abs().max()) < 2e-5 * max(1.0, float(att.grad.abs().max()))
    if names:
        for nm, dw in zip(names, dws):
            ref = w[nm].grad.reshape(dw.shape)
            assert float((dw.cpu().double() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), nm


# ---------------------------------------------------------------------------------------------
# fused per-clip tile operators (stair_tile_mlp_fwd, csrc/tile_mlp.hip) against the oracle's module operators
# ---------------------------------------------------------------------------------------------
P_ = 'submodules.'


def _tile_setup(T, n_tiles=5, seed=0):
    from stair_amd import synth
    config = dict(spec.DEFAULT_CONFIG)
    w = oracle_weights(config, seed)
    g = torch.Generator().manual_seed(100 + T)
    feat = torch.randn(n_tiles, T, 512, generator=g)
    dw = {k: v.to(DEV) for k, v in w.items() if k.startswith(P_) and not k.startswith(P_ + 'video_encoder')}
    return config, w, dw, feat, g


def _lin3(dw, prefix, act):
    return (dw[prefix + '.weight'], dw[prefix + '.bias'], act)


@pytest.mark.parametrize('T', [64, 40, 7])
def test_tile_localize_matches_oracle(T):
    """modules.py:199-217: video_linear (Lin . ReLU . Lin) on the tile + cosine against K keyword rows, K = 1 and 2 mixed,
    tiles gathered through an index (several instances read one clip)."""
    from stair_amd import ops
    config, w, dw, feat, g = _tile_setup(T)
    x_idx = torch.tensor([0, 3, 3, 1, 4, 2], dtype=torch.int32)
    K = [1, 2, 1, 2, 2, 1]
    kws = [torch.randn(k, 512, generator=g) for k in K]
    kb = torch.cat([O._lin(w, P_ + 'Localize.keyword_linear.0', kw) for kw in kws])           # keyword_linear rows (a separate small GEMM)
    first = np.concatenate([[0], np.cumsum(K)])[:-1]
    att = torch.zeros(sum(K) + 3, T, device=DEV)
    att_idx = torch.arange(sum(K), dtype=torch.int32) + 2
    i32 = lambda a: torch.as_tensor(np.asarray(a), dtype=torch.int32).to(DEV)
    saves, _ = ops.tile_mlp(feat.to(DEV), [_lin3(dw, P_ + 'Localize.video_linear.0', 'relu'), _lin3(dw, P_ + 'Localize.video_linear.3', None)],
                            'cosine', x_idx=x_idx.to(DEV), save=True, kb=kb.to(DEV), pair_first=i32(first), pair_cnt=i32(K),
                            att_idx=att_idx.to(DEV), att=att)
    for i in range(len(K)):
        ref = O.op_localize(w, feat[int(x_idx[i])], kws[i])
        got = att[2 + first[i]: 2 + first[i] + K[i]].cpu()
        assert float((got - ref).abs().max()) < 2e-5, i
        f1 = torch.relu(O._lin(w, P_ + 'Localize.video_linear.0', feat[int(x_idx[i])]))
        assert float((saves[0][i].cpu() - f1).abs().max()) < 1e-4 * max(1.0, float(f1.abs().max()))
        f2 = O._lin(w, P_ + 'Localize.video_linear.3', f1)
        assert float((saves[1][i].cpu() - f2).abs().max()) < 1e-4 * max(1.0, float(f2.abs().max()))
    assert float(att[:2].abs().max()) == 0.0 and float(att[2 + sum(K):].abs().max()) == 0.0      # nothing written outside the pairs' rows


@pytest.mark.parametrize('T', [64, 33])
@pytest.mark.parametrize('kw', ['representation', 'actions'])
def test_tile_filter_matches_oracle(T, kw):
    """modules.py:363-378 up to the sum over frames (its attention is identically 1), with per-instance clip lengths."""
    from stair_amd import ops
    config, w, dw, feat, g = _tile_setup(T, seed=1)
    lens = [T, max(1, T - 5), T, 1, T // 2]
    out = torch.empty(5, 512, device=DEV)
    pre = P_ + 'Filter.param.' + kw
    ops.tile_mlp(feat.to(DEV), [_lin3(dw, pre + '.0', 'relu'), _lin3(dw, pre + '.3', 'relu')], 'sum_rows', out=out, out_gstride=512,
                 len=torch.tensor(lens, dtype=torch.int32, device=DEV))
    for i in range(5):
        ref = O._mlp2(w, pre, feat[i][:lens[i]]).sum(0)
        assert float((out[i].cpu() - ref).abs().max()) < 2e-5 * max(1.0, float(ref.abs().max())), i


@pytest.mark.parametrize('T', [64, 24])
@pytest.mark.parametrize('tensor_kw', [True, False])
def test_tile_filterframe_matches_oracle(T, tensor_kw):
    """modules.py:399-414: three layers with the sigmoid attention between the second and the third."""
    from stair_amd import ops
    config, w, dw, feat, g = _tile_setup(T, seed=2)
    out = torch.zeros(7, T, 512, device=DEV)
    out_idx = torch.tensor([6, 0, 2, 5, 3], dtype=torch.int32, device=DEV)
    kind = 'representation' if tensor_kw else 'relations'
    pre = P_ + 'FilterFrame.param.' + kind
    layers = [_lin3(dw, pre + '.0', 'relu'), _lin3(dw, pre + '.3', 'relu'), _lin3(dw, P_ + 'FilterFrame.dense.0', 'relu')]
    kws = torch.randn(5, 512, generator=g)
    mid = None
    if tensor_kw:
        wa = dw[P_ + 'FilterFrame.attention.0.weight'].reshape(-1)
        extra = (kws.to(DEV) * wa[512:]).sum(1).contiguous()
        mid = (wa[:512].contiguous(), dw[P_ + 'FilterFrame.attention.0.bias'], extra)
    saves, rs = ops.tile_mlp(feat.to(DEV), layers, 'store', save=True, mid_rowdot=mid, out=out, out_idx=out_idx)
    for i in range(5):
        ref = O.op_filterframe(w, feat[i], kws[i] if tensor_kw else kind)
        got = out[int(out_idx[i])].cpu()
        assert float((got - ref).abs().max()) < 3e-5 * max(1.0, float(ref.abs().max())), i
        f = O._mlp2(w, pre, feat[i])
        assert float((saves[1][i].cpu() - f).abs().max()) < 1e-4 * max(1.0, float(f.abs().max()))          # f, NOT a_t f
        if tensor_kw:
            fk = torch.cat([f, kws[i].unsqueeze(0).expand(T, -1)], dim=1)
            a = torch.sigmoid(O._lin(w, P_ + 'FilterFrame.attention.0', fk)).reshape(-1)
            assert float((rs[i].cpu() - a).abs().max()) < 1e-5
    assert float(out[1].abs().max()) == 0.0 and float(out[4].abs().max()) == 0.0


@pytest.mark.parametrize('T', [64, 9])
def test_tile_hasitem_and_temporal_match_oracle(T):
    """modules.py:123-138 (Lin . ReLU + row-dot sigmoid) and :310-327 (row-scaled input, Lin . ReLU, LayerNorm)."""
    from stair_amd import ops
    config, w, dw, feat, g = _tile_setup(T, seed=3)
    att = torch.zeros(8, T, device=DEV)
    oi = torch.tensor([1, 7, 3, 4, 0], dtype=torch.int32, device=DEV)
    ops.tile_mlp(feat.to(DEV), [_lin3(dw, P_ + 'HasItem.param.0', 'relu')], 'rowdot_sigmoid', out=att, out_idx=oi, out_gstride=T,
                 vw=dw[P_ + 'HasItem.param.3.weight'].reshape(-1).contiguous(), vb=dw[P_ + 'HasItem.param.3.bias'])
    for i in range(5):
        assert float((att[int(oi[i])].cpu() - O.op_hasitem(w, feat[i]).reshape(T)).abs().max()) < 1e-5, i
    # Temporal's dense + LayerNorm on r_t feat_t (the relate net that produces r is its own kernel)
    r = torch.rand(6, T, generator=g)
    rs_idx = torch.tensor([5, 0, 2, 2, 1], dtype=torch.int32, device=DEV)
    out = torch.empty(5, T, 512, device=DEV)
    saves, _ = ops.tile_mlp(feat.to(DEV), [_lin3(dw, P_ + 'Temporal.dense.0', 'relu')], 'layernorm', row_scale=r.to(DEV), rs_idx=rs_idx, save=True,
                            out=out, gamma=dw[P_ + 'Temporal.layer_norm.weight'], beta=dw[P_ + 'Temporal.layer_norm.bias'], eps=1e-5)
    for i in range(5):
        ri = r[int(rs_idx[i])]
        y = torch.relu(O._lin(w, P_ + 'Temporal.dense.0', ri.unsqueeze(-1) * feat[i]))
        ref = torch.nn.functional.layer_norm(y, (512,), w[P_ + 'Temporal.layer_norm.weight'], w[P_ + 'Temporal.layer_norm.bias'], 1e-5)
        assert float((out[i].cpu() - ref).abs().max()) < 5e-5, i
        assert float((saves[0][i].cpu() - y).abs().max()) < 1e-4 * max(1.0, float(y.abs().max()))
