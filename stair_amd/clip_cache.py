"""Encode once, ask many: a library of clips run through the video bi-LSTM ahead of the questions.

The reference encodes the clip of every question again (/root/reference/video_nmn/module_net.py:74, encode_video :160-163); a
launch batch here shares a clip among its own questions only.  An evaluation run asks hundreds of thousands of questions about a
few thousand clips under one frozen checkpoint: ``VideoNMN.encode_clips`` fills a ``ClipCache`` (stair_encode_clips), and
``run_programs(..., clips=cache, video_index=rows)`` / ``forward_batch(batch, clip_cache=cache)`` then build plans without a video
encoder (STAIR_PLAN_VIDEO_ENCODED) whose first launch copies the cached rows into the plan's map arena.

The encodings belong to the weights and the matmul mode they were made with; ``ClipCache.check`` raises when either has changed.
"""
from __future__ import annotations

import numpy as np
import torch


class ClipCache:
    """[N, rows_cap, H] fp32 encodings on the device, the clips' frame counts, and an id -> row map.

    encode(video [n, T, V], lens (int32 numpy [n]), out ([n, rows_cap, H] view of the cache)) does the device work and stamp()
    returns (matmul mode, what identifies the state of the encoder weights); VideoNMN.encode_clips supplies both (tests of the
    bookkeeping supply stubs).  Rows are handed out in the order clips are added and never move."""

    def __init__(self, rows_cap, hidden_size, encode, stamp, device):
        self.rows_cap, self.hidden_size = int(rows_cap), int(hidden_size)
        self.device = torch.device(device)
        self._encode, self._stamp_fn = encode, stamp
        self._stamp = stamp()                # (matmul mode, state of the video-encoder weights) at creation
        self.matmul_mode = self._stamp[0]
        self._store = torch.empty(0, self.rows_cap, self.hidden_size, dtype=torch.float32, device=self.device)
        self._lens = []
        self._row = {}

    def __len__(self):
        return len(self._lens)

    def __contains__(self, clip_id):
        return clip_id in self._row

    @property
    def enc(self):
        """The encodings [N, rows_cap, H]; rows past a clip's length are zero.  A view: add() may move the storage."""
        return self._store[:len(self._lens)]

    @property
    def lengths(self):
        return np.asarray(self._lens, dtype=np.int32)

    def rows(self, ids):
        """Cache rows (int32 numpy) of the clips named `ids`; a missing id raises KeyError naming it."""
        out = np.empty(len(ids), dtype=np.int32)
        for i, k in enumerate(ids):
            if k not in self._row:
                raise KeyError('clip %r is not in the cache' % (k,))
            out[i] = self._row[k]
        return out

    def check(self):
        """ValueError when the encodings no longer belong to the model: its video-encoder weights were written or replaced since the
        cache was made (torch's tensor version counters and storage addresses: load_state_dict, optimizer steps, Trainer.step and
        in-place updates all move them; writes through `.data` or a raw pointer do not), or the matmul mode differs."""
        mode, weights = self._stamp_fn()
        if weights != self._stamp[1]:
            raise ValueError('the clip cache is stale: the video-encoder weights changed since the clips were encoded; re-encode '
                             'them (VideoNMN.encode_clips)')
        if mode != self._stamp[0]:
            raise ValueError('the clip cache was made under matmul mode %r, the model now runs %r; re-encode the clips '
                             '(VideoNMN.encode_clips)' % (self._stamp[0], mode))

    def _reserve(self, total):
        if total <= self._store.shape[0]:
            return
        grown = torch.empty(max(total, self._store.shape[0] * 3 // 2), self.rows_cap, self.hidden_size, dtype=torch.float32,
                            device=self.device)
        n = len(self._lens)
        if n:
            grown[:n].copy_(self._store[:n])
        self._store = grown

    def add(self, clips, ids=None, video_len=None, batch_size=1024):
        """Encode and append clips: a list of [L_i, V] tensors / arrays, or a padded [N, T, V] tensor with video_len [N] (None:
        every clip has T frames; the rows behind a clip's frames must hold finite values); fp32 or bf16 (all bf16: the stored
        clip-feature format, encoded from the bf16 rows).  ids: one hashable per clip (default: the row numbers).  Clips are
        encoded batch_size at a time, each chunk padded to its own longest clip.  Returns the new rows."""
        self.check()
        padded = isinstance(clips, torch.Tensor) and clips.dim() == 3
        if padded:
            lens = [int(clips.shape[1])] * clips.shape[0] if video_len is None else [int(x) for x in video_len]
            if len(lens) != clips.shape[0]:
                raise ValueError('video_len must have one entry per clip')
            if lens and (min(lens) < 1 or max(lens) > clips.shape[1]):
                raise ValueError('video_len must be in 1..T')
            dtype = clips.dtype
        else:
            if video_len is not None:
                raise ValueError('video_len belongs to a padded [N, T, V] tensor; a list of clips carries its own lengths')
            clips = [torch.as_tensor(c) for c in clips]
            if any(c.dim() != 2 for c in clips):
                raise ValueError('every clip must be [L, V]')
            lens = [int(c.shape[0]) for c in clips]
            dtype = torch.bfloat16 if clips and all(c.dtype == torch.bfloat16 for c in clips) else torch.float32
        if dtype != torch.bfloat16:
            dtype = torch.float32
        n, first = len(lens), len(self._lens)
        ids = list(range(first, first + n)) if ids is None else list(ids)
        if len(ids) != n:
            raise ValueError('one id per clip')
        if len(set(ids)) != n or any(k in self._row for k in ids):
            raise ValueError('clip ids must be new and distinct')
        if lens and (min(lens) < 1 or max(lens) > self.rows_cap):
            raise ValueError('every clip must have 1 <= L <= %d frames (the cache\'s rows_cap)' % self.rows_cap)
        self._reserve(first + n)
        step = max(1, int(batch_size))
        for s in range(0, n, step):
            clen = lens[s:s + step]
            T = max(clen)
            if padded:      # (the rows behind a clip's frames are the caller's padding: finite values)
                video = clips[s:s + step, :T].to(self.device, dtype)
            else:
                video = torch.stack([torch.nn.functional.pad(c.to(dtype), (0, 0, 0, T - c.shape[0])) for c in clips[s:s + step]]).to(self.device)
            self._encode(video.contiguous(), np.asarray(clen, dtype=np.int32), self._store[first + s: first + s + len(clen)])
        for k, L in zip(ids, lens):       # (recorded once every chunk has been enqueued: a failed add leaves the cache as it was)
            self._row[k] = len(self._lens)
            self._lens.append(L)
        return np.arange(first, first + n, dtype=np.int32)
