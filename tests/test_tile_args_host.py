"""Argument sets that stair_tile_mlp_fwd refuses (csrc/tile_mlp.hip: tile_mlp_check), each with the message it is refused with.
The check runs on the host before anything touches the device, and it never dereferences a pointer: the addresses below are
fake, non-null and 16-byte aligned.  The order of the checks decides which message a set gets, so every expectation is the
whole message.  No GPU."""
import pytest

from stair_amd._lib import lib, TileMlpArgs

NONE, STORE, SUM_ROWS, COSINE, ROWDOT_SIGMOID, LAYERNORM, ACCUMULATE, STORE_ROWS, ROWSCALE_ADJ = range(9)
P = [0x10000 + 0x100 * i for i in range(16)]        # fake device addresses
ODD = 0x20004                                       # ... and one that is not 16-byte aligned

MAP = dict(X=P[0], x_gstride=8 * 512, cnt=1, T=8, H=512, n_layers=1, W=(P[1],), act=(1,), tail=NONE)
VEC = dict(vec_pack=1, vec_cnt=64, cnt=1, T=64, H=512, pk_a=P[0], pk_b=P[2], n_layers=1, W=(P[1],), act=(1,), tail=STORE_ROWS,
           out=P[3], out_gstride=512, out_row_idx=P[4])
CHAIN = dict(MAP, act=(0,), tail=ACCUMULATE, out=P[3], out_gstride=8 * 512)
TEMPORAL = dict(MAP, act=(0,), ln_bwd=1, tail=ROWSCALE_ADJ, in_mask=P[5], in_mask_gstride=8 * 512, save_in=P[6], gamma=P[7],
                dgamma=P[8], dbeta=P[9], adj_feat=P[10], adj_feat_gstride=8 * 512, adj_rs=P[11], adj_drs=P[12], out=P[3],
                out_gstride=8 * 512)

# (id, arguments, message, split switch)
REFUSED = [
    ('hidden_size', dict(MAP, H=256), 'the fused tile operators are built for hidden_size 512', 1),
    ('no_layer', dict(MAP, n_layers=0), '1..3 layers', 1),
    ('four_layers', dict(MAP, n_layers=4), '1..3 layers', 1),
    ('vec_pack_4', dict(VEC, vec_pack=4), 'vec_pack: 1 [a, b], 2 [|a - b|, a, b], 3 [a, b, a * b]', 1),
    ('vec_no_operand', dict(VEC, pk_b=None), 'vector operands / cnt = ceil(vec_cnt / 64)', 1),
    ('vec_cnt', dict(VEC, vec_cnt=65), 'vector operands / cnt = ceil(vec_cnt / 64)', 1),
    ('vec_unaligned', dict(VEC, cat_save=ODD), 'vector operands must be 16-byte aligned', 1),
    ('vec_row_scale', dict(VEC, row_scale=P[5]), 'vector-level tiles take no map-level input options', 1),
    ('vec_in_mask', dict(VEC, in_mask=P[5]), 'vector-level tiles take no map-level input options', 1),
    ('vec_tail', dict(VEC, tail=STORE), 'vector-level tiles end in STORE_ROWS', 1),
    ('vec_act3', dict(VEC, act=(3,), act_mask=(P[5],)), 'no backward chains on vector-level tiles', 1),
    # the two classifications of a bucket (the check's and the launcher's) could have disagreed on these
    ('vec_in_bits', dict(VEC, in_bits=P[5]), 'chain options (act 3, in_mask, in_bits, x_broadcast, save_in, ACCUMULATE) are map-level', 1),
    ('vec_save_bits', dict(VEC, save_bits=(P[5],)), 'bit masks are a map-level option', 1),
    ('vec_act_bits', dict(VEC, act_bits=(P[5],)), 'act_bits belong to act 3', 1),
    ('vec_no_out', dict(VEC, out_row_idx=None), 'row-scatter tail: out, out_row_idx', 1),
    # ... and a well-formed set of the retired form is refused last of all
    ('vec_retired', dict(VEC), 'the vector-level form of the tile operator is retired (ABI 7): stair_vec_group runs these modules', 1),
    ('no_frames', dict(MAP, T=0), 'a tile holds 1..64 frames', 1),
    ('T65_split_off', dict(MAP, T=65, x_gstride=65 * 512), 'a tile holds 1..64 frames', 0),
    ('T142', dict(MAP, T=142, x_gstride=142 * 512), 'the tile operators take clips of at most 141 frames (64-row segments)', 1),
    ('T142_split_off', dict(MAP, T=142, x_gstride=142 * 512), 'a tile holds 1..64 frames', 0),
    ('null_input', dict(MAP, X=None), 'null input', 1),
    ('negative_cnt', dict(MAP, cnt=-1), 'null input', 1),
    ('store_rows_map', dict(MAP, tail=STORE_ROWS), 'STORE_ROWS is the vector-level tail', 1),
    ('ln_bwd_tail', dict(TEMPORAL, tail=STORE), 'ln_bwd and the ROWSCALE_ADJ tail come together (Temporal\'s backward chain)', 1),
    ('rowscale_adj_alone', dict(MAP, tail=ROWSCALE_ADJ), 'ln_bwd and the ROWSCALE_ADJ tail come together (Temporal\'s backward chain)', 1),
    ('ln_bwd_accumulate', dict(TEMPORAL, tail=ACCUMULATE), 'ln_bwd and the ROWSCALE_ADJ tail come together (Temporal\'s backward chain)', 1),
    ('ln_bwd_act3', dict(TEMPORAL, act=(3,), act_mask=(P[13],)), 'Temporal\'s backward chain is ONE transposed layer, no bias, no activation', 1),
    ('ln_bwd_two_layers', dict(TEMPORAL, n_layers=2, W=(P[1], P[1])), 'Temporal\'s backward chain is ONE transposed layer, no bias, no activation', 1),
    ('ln_bwd_vec', dict(VEC, ln_bwd=1, tail=ROWSCALE_ADJ), 'vector-level tiles end in STORE_ROWS', 1),
    ('ln_bwd_no_rows', dict(TEMPORAL, in_mask=None), 'ln_bwd: saved pre-LayerNorm rows (in_mask), gamma, dgamma, dbeta', 1),
    ('ln_bwd_row_scale', dict(TEMPORAL, row_scale=P[13]), 'ln_bwd takes no other input option', 1),
    ('ln_bwd_broadcast', dict(TEMPORAL, x_broadcast=1, x_gstride=512), 'ln_bwd takes no other input option', 1),
    # valid (save_in and in_mask belong to Temporal's chain, they are no chain options there) up to what comes later
    ('ln_bwd_no_adj_feat', dict(TEMPORAL, adj_feat=None), 'ROWSCALE_ADJ: adj_feat, adj_rs, adj_drs, out', 1),
    ('ln_bwd_unaligned', dict(TEMPORAL, gamma=ODD), 'ln_bwd operands must be 16-byte aligned', 1),
    ('ln_bwd_x_stride', dict(TEMPORAL, x_gstride=8 * 512 + 2), 'input tiles must be 16-byte aligned', 1),
    ('ln_bwd_in_bits', dict(TEMPORAL, in_mask=P[5], in_bits=P[13]), 'in_mask or in_bits, not both', 1),
    ('ln_bwd_act_bits', dict(TEMPORAL, act_bits=(P[13],)), 'act_bits belong to act 3', 1),
    ('ln_bwd_save_bits', dict(TEMPORAL, save_bits=(P[13],)), 'bit masks are a map-level option', 1),
    ('no_weights', dict(MAP, W=(None,)), 'weight planes (stair_pack_wfrag) missing or unaligned', 1),
    ('weights_unaligned', dict(MAP, n_layers=2, W=(P[1], ODD)), 'weight planes (stair_pack_wfrag) missing or unaligned', 1),
    ('act3_no_mask', dict(CHAIN, act=(3,)), 'act 3 multiplies by relu\'(act_mask[l]) (or its bits, act_bits[l])', 1),
    ('both_input_masks', dict(CHAIN, in_mask=P[5], in_bits=P[6]), 'in_mask or in_bits, not both', 1),
    ('chain_tail', dict(CHAIN, tail=COSINE, in_bits=P[5]), 'a backward chain ends in ACCUMULATE, STORE or NONE', 1),
    ('chain_row_scale', dict(CHAIN, row_scale=P[5]), 'a backward chain takes no row_scale / mid_rowdot / save_bits', 1),
    ('save_in_row_scale', dict(MAP, save_in=P[5], row_scale=P[6]), 'a backward chain takes no row_scale / mid_rowdot / save_bits', 1),
    ('act3_save_bits', dict(MAP, act=(3,), act_mask=(P[5],), save_bits=(P[6],)), 'a backward chain takes no row_scale / mid_rowdot / save_bits', 1),
    ('act_bits_forward', dict(MAP, act_bits=(P[5],)), 'act_bits belong to act 3', 1),
    ('broadcast_stride', dict(CHAIN, x_broadcast=1), 'a broadcast input is one [H] row per instance', 1),
    ('mid_rowdot_layers', dict(MAP, mid_rowdot=1, vw=P[5], vb=P[6]), 'mid_rowdot is FilterFrame\'s attention between layers 2 and 3', 1),
    ('input_unaligned', dict(MAP, X=ODD), 'input tiles must be 16-byte aligned', 1),
    ('input_stride', dict(MAP, x_gstride=8 * 512 + 1), 'input tiles must be 16-byte aligned', 1),
    ('store_no_out', dict(MAP, tail=STORE), 'out missing or unaligned', 1),
    ('sum_rows_stride', dict(MAP, tail=SUM_ROWS, out=P[3], out_gstride=510), 'out missing or unaligned', 1),
    ('accumulate_unaligned', dict(CHAIN, out=ODD), 'out missing or unaligned', 1),
    ('T65_chain_no_out', dict(CHAIN, T=65, x_gstride=65 * 512, out=None), 'out missing or unaligned', 1),
    ('cosine_tables', dict(MAP, tail=COSINE, kb=P[5], pair_first=P[6], pair_cnt=P[7], att=P[8]), 'cosine tail: keyword rows / pair tables / att', 1),
    ('rowdot_no_vb', dict(MAP, tail=ROWDOT_SIGMOID, vw=P[5], out=P[3]), 'row-dot tail: vw, vb, out', 1),
    ('layernorm_no_beta', dict(MAP, tail=LAYERNORM, gamma=P[5], out=P[3], out_gstride=8 * 512), 'LayerNorm tail: gamma, beta, out', 1),
    ('unknown_tail', dict(MAP, tail=9), 'unknown tail', 1),
]


@pytest.fixture(autouse=True)
def default_switch():
    yield
    lib.stair_set_tile_split(-1)


def _args(fields):
    a = TileMlpArgs()
    for k, v in fields.items():
        if isinstance(v, tuple):
            for i, x in enumerate(v):
                getattr(a, k)[i] = x
        else:
            setattr(a, k, v)
    return a


@pytest.mark.parametrize('fields,message,split', [pytest.param(*c[1:], id=c[0]) for c in REFUSED])
def test_refused_with_its_message(fields, message, split):
    assert lib.stair_set_tile_split(split) == 0
    a = _args(fields)
    assert lib.stair_tile_mlp_fwd(a, None) != 0
    assert lib.stair_last_error().decode() == 'tile_mlp_check: ' + message


def test_null_args():
    assert lib.stair_tile_mlp_fwd(None, None) != 0
    assert lib.stair_last_error().decode() == 'stair_tile_mlp_fwd: null args'
