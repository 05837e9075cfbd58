"""Upload once, name by row: the raw clip features of a dataset kept on the device.

A training run whose video encoder learns cannot use a ``ClipCache`` (the encodings would be stale after the first step), and packing
the dense ``[n_clips, T, V]`` tensor on the host for every window moves hundreds of megabytes per step.  The features themselves never
change: a ``ClipLibrary`` holds them on the device, ``run_programs(library=lib, video_index=rows)`` / ``Trainer.step(library=lib, ...)``
name clips by library row, and one launch (stair_gather_clips) writes the dense tensor the encoder reads.  A step then uploads the
rows and lengths of its clips -- a few kilobytes.

The bookkeeping is ``ClipCache``'s without a stamp: raw features do not depend on weights.
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch


class ClipLibrary:
    """[N, rows_cap, V] clip features on the device, all bf16 or all fp32 (fixed when the library is made), the clips' frame counts,
    and an id -> row map.  Rows are handed out in the order clips are added and never move; behind a clip's frames the store holds
    zeros whatever the caller's padding held."""

    def __init__(self, rows_cap, video_size, device, dtype=torch.float32):
        if dtype not in (torch.float32, torch.bfloat16):
            raise ValueError('a clip library holds float32 or bfloat16 features, got %s' % (dtype,))
        self.rows_cap, self.video_size = int(rows_cap), int(video_size)
        if self.rows_cap < 1 or self.video_size < 1 or self.video_size * (2 if dtype == torch.bfloat16 else 4) % 16:
            raise ValueError('rows_cap must be positive and a frame a multiple of 16 bytes (video_size % 4 == 0, bf16: % 8 == 0)')
        self.device, self.dtype = torch.device(device), dtype
        self._store = torch.empty(0, self.rows_cap, self.video_size, dtype=dtype, device=self.device)
        self._lens = []
        self._row = {}

    @classmethod
    def from_clips(cls, clips, device, dtype=None, rows_cap=None):
        """The library of a {video_id: [L, V] tensor} dict (data.load_clip_features), rows in the dict's order, ids its keys.
        dtype: torch.float32 / torch.bfloat16 (default: bf16 when every clip is bf16, else fp32); rows_cap: the longest clip."""
        ids = list(clips)
        tensors = [torch.as_tensor(clips[k]) for k in ids]
        if not tensors:
            raise ValueError('from_clips needs at least one clip (its shape sizes the library)')
        if dtype is None:
            dtype = torch.bfloat16 if all(c.dtype == torch.bfloat16 for c in tensors) else torch.float32
        lib_ = cls(rows_cap or max(int(c.shape[0]) for c in tensors), int(tensors[0].shape[-1]), device, dtype)
        lib_.add([c.to(dtype) for c in tensors], ids=ids)
        return lib_

    def __len__(self):
        return len(self._lens)

    def __contains__(self, clip_id):
        return clip_id in self._row

    @property
    def clips(self):
        """The features [N, rows_cap, V]; frames past a clip's length are zero.  A view: add() may move the storage."""
        return self._store[:len(self._lens)]

    @property
    def ids(self):
        """The clips' ids in row order."""
        return list(self._row)

    @property
    def lengths(self):
        return np.asarray(self._lens, dtype=np.int32)

    def rows(self, ids):
        """Library rows (int32 numpy) of the clips named `ids`; a missing id raises KeyError naming it."""
        out = np.empty(len(ids), dtype=np.int32)
        for i, k in enumerate(ids):
            if k not in self._row:
                raise KeyError('clip %r is not in the library' % (k,))
            out[i] = self._row[k]
        return out

    def _reserve(self, total):
        if total <= self._store.shape[0]:
            return
        grown = torch.empty(max(total, self._store.shape[0] * 3 // 2), self.rows_cap, self.video_size, dtype=self.dtype, device=self.device)
        n = len(self._lens)
        if n:
            grown[:n].copy_(self._store[:n])
        self._store = grown

    def add(self, clips, ids=None, video_len=None, batch_size=1024):
        """Append clips: a list of [L_i, V] tensors / arrays, or a padded [N, T, V] tensor with video_len [N] (None: every clip has
        T frames; what the padding holds does not matter, the store gets zeros there).  Every clip must have the library's dtype
        (a library is all bf16 or all fp32: rounding is the caller's decision, data.load_clip_features(dtype='bf16')).  ids: one
        hashable per clip (default: the row numbers).  Clips are staged and copied batch_size at a time.  Returns the new rows."""
        padded = isinstance(clips, torch.Tensor) and clips.dim() == 3
        if padded:
            lens = [int(clips.shape[1])] * clips.shape[0] if video_len is None else [int(x) for x in video_len]
            if len(lens) != clips.shape[0]:
                raise ValueError('video_len must have one entry per clip')
            if lens and (min(lens) < 1 or max(lens) > clips.shape[1]):
                raise ValueError('video_len must be in 1..T')
            dtypes, widths = {clips.dtype}, {int(clips.shape[2])}
        else:
            if video_len is not None:
                raise ValueError('video_len belongs to a padded [N, T, V] tensor; a list of clips carries its own lengths')
            clips = [torch.as_tensor(c) for c in clips]
            if any(c.dim() != 2 for c in clips):
                raise ValueError('every clip must be [L, V]')
            lens = [int(c.shape[0]) for c in clips]
            dtypes, widths = {c.dtype for c in clips}, {int(c.shape[1]) for c in clips}
        if dtypes - {self.dtype}:
            raise ValueError('mixed dtypes: the library holds %s, the clips are %s (a library is all bf16 or all fp32)'
                             % (self.dtype, ', '.join(sorted(str(d) for d in dtypes))))
        if widths - {self.video_size}:
            raise ValueError('clips must have video_size = %d features per frame' % self.video_size)
        n, first = len(lens), len(self._lens)
        ids = list(range(first, first + n)) if ids is None else list(ids)
        if len(ids) != n:
            raise ValueError('one id per clip')
        if len(set(ids)) != n or any(k in self._row for k in ids):
            raise ValueError('clip ids must be new and distinct')
        if lens and (min(lens) < 1 or max(lens) > self.rows_cap):
            raise ValueError('every clip must have 1 <= L <= %d frames (the library\'s rows_cap)' % self.rows_cap)
        self._reserve(first + n)
        step = max(1, int(batch_size))
        for s in range(0, n, step):
            clen = lens[s:s + step]
            stage = torch.zeros(len(clen), self.rows_cap, self.video_size, dtype=self.dtype)      # zeros behind every clip's end
            for i, L in enumerate(clen):
                stage[i, :L] = clips[s + i][:L]
            self._store[first + s: first + s + len(clen)].copy_(stage)
        for k, L in zip(ids, lens):       # (recorded once every chunk has been copied: a failed add leaves the library as it was)
            self._row[k] = len(self._lens)
            self._lens.append(L)
        return np.arange(first, first + n, dtype=np.int32)

    def gather(self, rows, lens, T, out=None):
        """Dense [n, T, V] clips of the DEVICE int32 arrays rows / lens (lens None: every clip min(rows_cap, T) frames) on the current
        stream (stair_gather_clips): the first lens[v] frames of library row rows[v], zeros behind them.  The caller has checked the
        host copies: rows inside the library, 1 <= lens <= min(rows_cap, T)."""
        from ._lib import check, lib
        n = int(rows.shape[0])
        if out is None:
            out = torch.empty(n, int(T), self.video_size, dtype=self.dtype, device=self.device)
        check(lib.stair_gather_clips(C.c_void_p(self._store.data_ptr()), self._store.element_size(), self.rows_cap * self.video_size,
                                     self.rows_cap, self.video_size, C.c_void_p(rows.data_ptr()),
                                     C.c_void_p(lens.data_ptr() if lens is not None else None), n, int(T), C.c_void_p(out.data_ptr()),
                                     C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return out
