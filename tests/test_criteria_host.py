"""Host halves of the intermediate-supervision criteria (stair_amd/losses.py) against the oracle (oracle/nmn_losses.py)
and the reference's own FilterFrame values (tests/golden/criteria_filterframe.npz).  CPU only."""
import json
import math
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import nmn_losses as OL
from stair_amd import losses as SL
from helpers import GOLDEN


def intervals(L):
    """(start, end) pairs at clip length L: integer endpoints, zero length, inside one frame, reversed, start < 0, end > L,
    start >= L, and negative ends down to floor(end) = -L (the reference's index then counts from the clip's end)."""
    out = [(0.0, float(L)), (float(L // 4), float(max(L // 4 + 1, 3 * L // 4))), (0.37 * L, 0.37 * L), (float(L // 2),) * 2,
           (L // 3 + 0.2, L // 3 + 0.7), (0.8 * L, 0.2 * L), (-3.5, 0.6 * L), (0.3 * L, L + 5.2), (float(L), L + 1.0),
           (L + 0.5, L + 3.0), (-1.0, -0.5), (3.0, -2.0), (-3.0, -1.0), (0.5 * L, -float(L)), (-2.0, -0.4 * L),
           (5.0, 5.0), (7.0, 9.0), (-1.0, 0.4), (L - 0.5, L + 1.0)]
    return [iv for iv in out if math.floor(min(L - 0.001, iv[1])) >= -L]


@pytest.mark.parametrize('L', [1, 2, 8, 40, 63, 64, 65, 100])
def test_span_mask_matches_oracle_span_to_attention(L):
    """losses._span_mask (the FilterFrame target of the host) == the oracle's span_to_attention, bit for bit."""
    for iv in intervals(L):
        got = SL._span_mask(iv[0], iv[1], L)
        ref = OL.span_to_attention(iv, L).numpy()
        assert got.dtype == np.float32 and np.array_equal(got, ref), (L, iv, got, ref)


def test_span_mask_negative_ends_wrap_like_the_reference():
    """The table of the negative-end divergence at L = 8: the frame L + floor(end) takes end - start."""
    for iv, frame, value in (((-1.0, -0.5), 7, -0.501), ((3.0, -2.0), 6, -5.0), ((-3.0, -1.0), 7, -1.001)):
        g = SL._span_mask(iv[0], iv[1], 8)
        want = np.zeros(8, dtype=np.float32)
        want[frame] = value
        assert np.array_equal(g, want), (iv, g)


def test_filterframe_target_reproduces_reference_losses():
    """losses.filterframe_target fed through BCELoss(softmax(pred)) gives the reference's loss for every case of
    criteria_filterframe.npz (shared object ids, an empty gold, intervals past both clip ends included)."""
    z = np.load(os.path.join(GOLDEN, 'criteria_filterframe.npz'))
    meta = json.loads(bytes(z['meta']).decode())
    index = SL.object_index(meta['word2id'])
    assert index == meta['word2index']
    for i, case in enumerate(meta['cases']):
        pred = torch.from_numpy(z['c%d/pred' % i])
        gold = {k: tuple(v) for k, v in case['gold'].items()}
        tgt = torch.from_numpy(SL.filterframe_target(gold, case['T'], meta['O'], index))
        loss = float(F.binary_cross_entropy(torch.softmax(pred, dim=1), tgt))
        ref = float(z['c%d/loss' % i])
        assert abs(loss - ref) <= 1e-6 * max(1.0, abs(ref)), (i, loss, ref)


@pytest.mark.parametrize('L', [1, 8, 40])
def test_unindexable_gold_ends_are_refused_where_the_reference_raises(L):
    """The reference indexes gold_tensor[floor(end)]: floor(end) < -L is an IndexError there.  The host refuses exactly
    those golds, with a ValueError that names the node; every other end is accepted."""
    ends = [-L - 0.5, -L - 1.0, -2.0 * L - 3.0, -L - 1e-9, -float(L), -L + 0.5, -0.5, 0.0, L + 3.0]
    for end in ends:
        try:
            OL.span_to_attention((0.5, end), L)
            ref_raises = False
        except IndexError:
            ref_raises = True
        if ref_raises:
            with pytest.raises(ValueError, match='Temporal at program position 3 of question 5'):
                SL.refuse_unindexable_ends([0.0, end], [L, L], lambda j: 'Temporal at program position 3 of question 5')
        else:
            SL.refuse_unindexable_ends([end], [L], lambda j: 'unused')
    # per-interval clip lengths: the same end is fine on a long clip and refused on a short one
    SL.refuse_unindexable_ends([-5.0, -5.0], [40, 5], lambda j: 'unused')
    with pytest.raises(ValueError, match='interval 1'):
        SL.refuse_unindexable_ends([-5.0, -5.0], [40, 4], lambda j: 'interval %d' % j)
