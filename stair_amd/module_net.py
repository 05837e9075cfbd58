"""Host-side mirror of the reference's ``video_nmn/module_net.py``: a ``VideoNMN`` with the same
constructor, ``forward(data, ...)`` contract, ``state_dict`` keys and helper entry points
(/root/reference/video_nmn/module_net.py:11-216), executing on libstair_hip.so.

Differences that matter to a caller:

* ``forward_batch`` runs MANY questions in one pass (the reference is batch-1 by construction,
  train_module.py:282); ``forward(data)`` is the drop-in single-question form built on it.
* ``forward`` builds no autograd graph: training goes through ``run_programs(train=True)`` + ``BatchResult.backward`` (HIP
  backward kernels) driven by ``stair_amd.train.Trainer``, where the decoder cross-entropy loss is built in.  ``logits(...)``
  is the differentiable form (stair_amd/autograd.py): any loss on the logits, gradients for parameters and inputs.
* programs whose operand kinds do not fit a module raise ``StairError`` at plan-build time instead
  of a torch shape error in the middle of execution.

torch is plumbing here (device memory, streams, Parameter containers); the arithmetic is HIP.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Any, NamedTuple, Optional

import numpy as np
import torch
from torch import nn

from . import frontend, ops, spec
from ._lib import PlanInfo, StairConfig, StairError, check, lib

VAL_STR, VAL_VEC, VAL_MAP, VAL_ATT, VAL_FRAME, VAL_PAIR = range(6)
RUN_INDEX_RESIDENT, RUN_VIDEO_BF16, RUN_PROJECTED = 1, 2, 4          # stair_plan_run_flags / stair_plan_backward flags (include/stair_hip.h)
PLAN_EXT_PROJECTION, PLAN_VIDEO_ENCODED = 4, 8                       # stair_plan_build* flags


class ClipSource(NamedTuple):
    """Where a plan's clip tiles come from: clip features that the plan's own video encoder reads (`video`), or encodings made
    before -- a ClipCache's or the caller's own (`enc`) -- of which the plan gathers the rows `rows` and runs no video encoder.
    Made by VideoNMN._clip_source, which carries the checks of each form; the pass (VideoNMN._run) only reads it."""
    video: Optional[torch.Tensor]       # [n_videos, T, V] clip features, fp32 or bf16; None on encoded clips
    enc: Optional[torch.Tensor]         # [n_clips, rows_cap, H] encodings the plan gathers from; None on clip features
    cache: Any                          # the ClipCache that owns enc, kept alive for the plan (it holds enc's address); else None
    rows: Optional[np.ndarray]          # int32 [n_videos]: the row of enc of every plan clip (map slot v = row rows[v]); else None
    n_videos: int                       # clips of the plan
    index: Optional[np.ndarray]         # int32 [n]: the plan clip of every question; None: question q asks about clip q
    lens: Optional[np.ndarray]          # int32 [n_videos]: frames of every plan clip; None: all of them have T
    T: int
    # clips named by ClipLibrary row (run_programs(library=...)): the library and the row of every plan clip.  Until the pass has
    # gathered them `video` is None; from then on it is the dense [n_videos, T, V] staging tensor and the source reads like one
    # made of clip features (VideoNMN._gathered)
    library: Any = None
    library_rows: Optional[np.ndarray] = None

    def video_arg(self):
        """(the clip features' address or NULL, RUN_VIDEO_BF16 or 0): the video arguments of every run and reverse-pass call."""
        v = self.video
        return C.c_void_p(v.data_ptr() if v is not None else None), RUN_VIDEO_BF16 if v is not None and v.dtype == torch.bfloat16 else 0

    def with_tensor(self, t):
        """The same source reading its tensor -- the clip features, else the encodings -- from `t` (autograd hands in a detached one)."""
        return self._replace(video=t) if self.video is not None else self._replace(enc=t)

    def question_frames(self):
        """[n] frames of every question's clip when the clips differ in length, else None (all T)."""
        if self.lens is None:
            return None
        return self.lens[self.index] if self.index is not None else self.lens


class L2Normalize(nn.Module):
    """module_net.py:211-216."""

    def forward(self, feat):
        return ops.l2normalize(feat)


class _Node(nn.Module):
    """Parameter container reproducing the reference's attribute paths (``param.representation.0`` ...).
    Calling a node that holds ``weight``/``bias`` applies it as a Linear (used for pretrain heads)."""

    def __getitem__(self, key):
        return self._modules[str(key)]

    def forward(self, x):
        return ops.linear(x, self.weight, self.bias)


class _TemporalNode(_Node):
    """TemporalModule.pretrain_head returns the relate output of the LAST call (modules.py:285-288)."""
    related_attn = None

    def pretrain_head(self, *args):
        return self.related_attn


def _init_param(name, p, config):
    H = config['hidden_size']
    with torch.no_grad():
        if name.endswith('layer_norm.weight'):
            p.fill_(1.0)
        elif name.endswith('layer_norm.bias'):
            p.zero_()
        elif name.endswith('Relate.beta'):
            p.uniform_(0.0, 1.0)                                   # torch.rand, modules.py:420
        elif '_encoder.' in name:
            b = 1.0 / math.sqrt(H // 2)
            p.uniform_(-b, b)                                      # nn.LSTM default
        else:
            table = dict(spec.weight_table(config))
            wshape = table[name[:-5] + '.weight'] if name.endswith('.bias') else tuple(p.shape)
            b = 1.0 / math.sqrt(int(np.prod(wshape[1:])))
            p.uniform_(-b, b)                                      # nn.Linear / nn.Conv1d default


class _IndexRing:
    """Host int32 arrays -> the device through a ring of page-locked buffers, without a synchronise: the host waits only for the
    copy issued `depth` uploads ago (the reasoning of train._PinnedRing; the buffers here grow with the arrays)."""

    def __init__(self, depth=8):
        self.bufs, self.events, self.i = [None] * depth, [None] * depth, 0

    def upload(self, values, device):
        k = self.i
        self.i = (k + 1) % len(self.bufs)
        if self.events[k] is not None:
            self.events[k].synchronize()
        n = int(values.shape[0])
        if self.bufs[k] is None or self.bufs[k].numel() < n:
            self.bufs[k] = torch.empty(max(n * 3 // 2, 256), dtype=torch.int32).pin_memory()
        host = self.bufs[k][:n]
        host.copy_(torch.from_numpy(values))
        t = host.to(device, non_blocking=True)
        self.events[k] = torch.cuda.Event()
        self.events[k].record()
        return t


def _clip_key(x):
    """Identity of a clip's feature buffer: same storage, offset and shape = same clip."""
    if isinstance(x, torch.Tensor):
        return ('t', x.untyped_storage().data_ptr(), x.storage_offset(), tuple(x.shape), tuple(x.stride()))
    if isinstance(x, np.ndarray):
        return ('n', x.__array_interface__['data'][0], x.shape, x.strides)
    return ('o', id(x))


class BatchResult:
    """Outputs of one batched pass plus read access to every intermediate program value.

    `logits` and `pred` are tensors of their own.  Everything else -- node(), related_attn(), token_feature,
    question_feature, grad_arena() -- is a VIEW into the model's shared workspace and is overwritten by the next
    run_programs / forward_batch / Trainer.step on the same model: clone what must outlive it (VideoNMN.forward does)."""

    def __init__(self, model, plan, info, ws, logits, pred, prog_off, programs, src, question, proj):
        self._model, self._plan, self.info, self._ws = model, plan, info, ws
        self.logits, self.pred = logits, pred
        self._prog_off, self._programs = prog_off, programs
        self._src, self._question, self._proj = src, question, proj
        self._video = src.video
        self.question_frames = src.question_frames()    # the loss driver masks its criteria with them
        # a pass on encoded clips (run_programs(clips=...), logits(encoded=...)): the cache and the encodings, kept alive for the plan
        # (it holds their address), and the row of every plan clip (map slot v = row clip_rows[v]); video is None then
        self._clips, self._enc, self.clip_rows = src.cache, src.enc, src.rows

    def status_word(self):
        """The plan's status word (int32 view of one workspace element): 0 = every pass on this workspace since run_programs
        completed normally; 1 = a cooperative recurrence timed out (stair_lstm_args.status) and the results hold NaN."""
        off = self.info.status_off
        return self._ws[off: off + 1].view(torch.int32)

    def check(self):
        """Synchronises and raises StairError when a pass of this batch reported a failure (stair_plan_status)."""
        check(lib.stair_plan_status(self._plan, C.c_void_p(self._ws.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def zero_grad_arenas(self):
        check(lib.stair_plan_zero_grads(self._plan, C.c_void_p(self._ws.data_ptr()),
                                        C.c_void_p(torch.cuda.current_stream().cuda_stream)))

    def grad_arena(self, kind):
        """View of a gradient arena ('vec' [n_vec,H], 'map' [n_map,T,H], 'att' [n_att,T]) of a training plan."""
        H, T, inf = self._model.config['hidden_size'], self.info.T, self.info
        if kind == 'vec':
            return self._ws[inf.gvec_off: inf.gvec_off + inf.n_vec * H].view(inf.n_vec, H)
        if kind == 'map':
            return self._ws[inf.gmap_off: inf.gmap_off + inf.n_map * T * H].view(inf.n_map, T, H)
        return self._ws[inf.gatt_off: inf.gatt_off + inf.n_att * T].view(inf.n_att, T)

    def backward(self, answers, loss_scale=1.0, keep_arenas=False, ready_event=None):
        """Reverse pass of a train=True run: decoder cross entropy against `answers` (int32 [n] on the GPU),
        gradients of loss_scale * sum_i CE_i accumulated into the model's gradient buffers.
        keep_arenas: the gradient arenas were zeroed by zero_grad_arenas() and hold injected loss gradients.
        ready_event: a torch.cuda.Event that has been recorded once (so that its hipEvent_t exists); the pass records it on the
        current stream when every gradient except the two encoders' is final (stair_plan_set_backward_event).
        Returns the unscaled per-question losses [n]."""
        ops._req(answers, 'answers', torch.int32)
        loss = torch.empty(self.info.n_questions, dtype=torch.float32, device=answers.device)
        self._model._bind_grads()
        video, bf16 = self._src.video_arg()     # NULL: a training plan of encoded clips (no clip features, no video encoder)
        check(lib.stair_plan_set_backward_event(self._plan, C.c_void_p(ready_event.cuda_event if ready_event is not None else None)))
        check(lib.stair_plan_backward(self._model._ctx, self._plan, video,
                                      C.c_void_p(self._question.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                      self._ws.numel() * 4, C.c_void_p(answers.data_ptr()), C.c_float(loss_scale),
                                      C.c_void_p(loss.data_ptr()), (1 if keep_arenas else 0) | bf16,
                                      C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        return loss

    def backward_dlogits(self, d_logits, d_video=None, d_question=None, keep_arenas=False, bind_grads=True, d_encoded=None):
        """Reverse pass of a train=True run seeded by an arbitrary logits gradient (stair_plan_backward_dlogits): d_logits
        float32 [n, A] on the GPU, already scaled.  Parameter gradients are accumulated into the model's gradient buffers
        (bind_grads=False: into the buffers the caller bound with stair_ctx_set_grad).  d_video (float32, the shape of the
        run's video) and d_question (float32 [q_rows, E]) are optional and OVERWRITTEN with the input gradients.  The pass
        overwrites the plan's saved gates: a batch goes backward once.
        A pass on encoded clips (run_programs(clips=...) / the `encoded=` form of VideoNMN.logits) has no video: d_video must be
        None.  d_encoded (optional, float32, the shape of the encodings the plan reads) receives the gradient of the encodings
        (stair_plan_set_encoded_video_grad): the rows of the plan's clips (clip_rows) are OVERWRITTEN -- a clip's gradient summed
        over the questions that share it, zeros behind its frames -- and every other row is left as it is."""
        n, A = self.info.n_questions, self._model.config['answer_vocab_length']
        if self._video is None and d_video is not None:
            raise ValueError('a pass on encoded clips has no video to send a gradient to (d_encoded is the gradient of the encodings)')
        if d_encoded is not None:
            if self._enc is None:
                raise ValueError('d_encoded belongs to a pass on encoded clips')
            ops._req(d_encoded, 'd_encoded')
            if tuple(d_encoded.shape) != tuple(self._enc.shape):
                raise ValueError('d_encoded must have the shape of the encodings %s' % (tuple(self._enc.shape),))
        ops._req(d_logits, 'd_logits')
        if tuple(d_logits.shape) != (n, A):
            raise ValueError('d_logits must be [%d, %d]' % (n, A))
        if d_video is not None:
            ops._req(d_video, 'd_video')
            if tuple(d_video.shape) != tuple(self._video.shape):
                raise ValueError('d_video must have the shape of the video %s' % (tuple(self._video.shape),))
        if d_question is not None:
            ops._req(d_question, 'd_question')
            if tuple(d_question.shape) != tuple(self._question.shape):
                raise ValueError('d_question must have the shape of the question rows %s' % (tuple(self._question.shape),))
        if bind_grads:
            self._model._bind_grads()
        video, bf16 = self._src.video_arg()
        ptr = lambda t: C.c_void_p(t.data_ptr() if t is not None else None)
        if d_encoded is not None:       # the request: the plan keeps the pointer for this pass only
            cap, H = self._enc.shape[1], self._enc.shape[2]
            check(lib.stair_plan_set_encoded_video_grad(self._plan, ptr(d_encoded), cap * H, cap))
        try:
            check(lib.stair_plan_backward_dlogits(self._model._ctx, self._plan, video, ptr(self._question), ptr(self._ws),
                                                  self._ws.numel() * 4, ptr(d_logits), ptr(d_video), ptr(d_question),
                                                  (1 if keep_arenas else 0) | bf16,
                                                  C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        finally:
            if d_encoded is not None:
                check(lib.stair_plan_set_encoded_video_grad(self._plan, None, 0, 0))

    def capture_graph(self):
        """Record this batch's forward pass (encoders, every program level, decoder, argmax) into a hipGraph and
        return a CapturedPlan whose replay() re-runs it with ONE launch -- BASELINE.json configs[3].  The graph
        reads self's video / question tensors and writes self.logits / self.pred in place: copy new inputs into
        those tensors (same programs, spans and lengths -- i.e. the same plan) and replay.  The plan gets a
        private workspace, because the model's shared one is rewritten by every other batch."""
        if self.info.gvec_off >= 0:
            raise StairError('capture_graph is for inference plans')
        return CapturedPlan(self)

    def touched(self):
        """bool per canonical weight: does this batch's program mix send a gradient into it?"""
        n = len(self._model._weight_names)
        arr = (C.c_int32 * n)()
        check(lib.stair_plan_touched(self._model._ctx, self._plan, arr, n))
        return [bool(v) for v in arr]

    def __del__(self):
        if getattr(self, '_plan', None):
            lib.stair_plan_destroy(self._plan)
            self._plan = None

    def _arena(self, off, rows, cols):
        return self._ws[off: off + rows * cols].view(rows, cols)

    def node_table(self):
        """(kind, slot, aux, level, rel_slot) of EVERY program token of the batch as int32 numpy arrays indexed by
        prog_off[q] + i -- one library call (stair_plan_nodes) instead of one per node."""
        tab = getattr(self, '_node_table', None)
        if tab is None:
            n = self.info.n_nodes
            tab = tuple(np.empty(n, dtype=np.int32) for _ in range(5))
            ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
            check(lib.stair_plan_nodes(self._plan, ip(tab[0]), ip(tab[1]), ip(tab[2]), ip(tab[3]), ip(tab[4]), n))
            self._node_table = tab
        return tab

    def node_info(self, q, i):
        k, s, a, l, r = (C.c_int32() for _ in range(5))
        check(lib.stair_plan_node(self._plan, int(self._prog_off[q] + i), C.byref(k), C.byref(s), C.byref(a),
                                  C.byref(l), C.byref(r)))
        return k.value, s.value, a.value, l.value, r.value

    def node(self, q, i):
        """Value of token i of question q: a str for keywords, else a tensor VIEW into the workspace."""
        H, T, inf = self._model.config['hidden_size'], self.info.T, self.info
        kind, slot, aux, _, _ = self.node_info(q, i)
        if kind == VAL_STR:
            return self._programs[q][i]
        if kind == VAL_VEC:
            return self._arena(inf.vec_off, inf.n_vec, H)[slot]
        if kind == VAL_MAP:
            return self._ws[inf.map_off: inf.map_off + inf.n_map * T * H].view(inf.n_map, T, H)[slot]
        if kind == VAL_ATT:
            return self._arena(inf.att_off, inf.n_att, T)[slot: slot + aux]
        if kind == VAL_FRAME:
            return self._arena(inf.att_off, inf.n_att, T)[slot]
        if kind == VAL_PAIR:
            v = self._arena(inf.vec_off, inf.n_vec, H)
            return torch.stack([v[slot], v[aux]])
        raise StairError('node has no value')

    def saved(self, q, i, which=0):
        """Training plans: view of the activation the backward pass keeps for token i of question q (stair_plan_saved_offset):
        [T,H] tiles of the tile MLPs, the [H] hidden row of Exists / ToAction; i = None: the decoder's hidden row [2H].
        None when the node keeps no such buffer."""
        H, T = self._model.config['hidden_size'], self.info.T
        tok = -1 - q if i is None else int(self._prog_off[q] + i)
        off = C.c_int64(-1)
        check(lib.stair_plan_saved_offset(self._plan, tok, which, C.byref(off)))
        if off.value < 0:
            return None
        if i is None:
            return self._ws[off.value: off.value + 2 * H]
        if self._programs[q][i] in ('Exists', 'ToAction'):
            return self._ws[off.value: off.value + H]
        return self._ws[off.value: off.value + T * H].view(T, H)

    def related_attn(self, q, i):
        _, _, _, _, rel = self.node_info(q, i)
        return self._arena(self.info.att_off, self.info.n_att, self.info.T)[rel] if rel >= 0 else None

    def levels(self, q):
        return [self.node_info(q, i)[3] for i in range(len(self._programs[q]))]

    @property
    def token_feature(self):
        return self._arena(self.info.tok_off, self.info.n_tok_rows, self._model.config['hidden_size'])

    @property
    def question_feature(self):
        return self._arena(self.info.qfeat_off, self.info.n_questions, self._model.config['hidden_size'])


class CapturedPlan:
    """A plan's forward pass as a replayable hipGraph (torch.cuda.CUDAGraph on ROCm).  Holds the BatchResult (plan,
    static input/output tensors) and its own workspace alive."""

    def __init__(self, res):
        self.result = res
        model, info = res._model, res.info
        dev = res._question.device
        self._ws = torch.empty((info.workspace_bytes + 3) // 4, dtype=torch.float32, device=dev)
        self._proj = None
        if res._proj is not None:       # the plan keeps its projections outside the workspace: a private buffer too
            self._proj = torch.empty(res._proj.numel(), dtype=torch.float32, device=dev)     # (the replay recomputes them: no RUN_PROJECTED)
            check(lib.stair_plan_set_projection(model._ctx, res._plan, C.c_void_p(self._proj.data_ptr()), self._proj.numel()))
        self.logits, self.pred = res.logits, res.pred
        side = torch.cuda.Stream(device=dev)
        side.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(side):
            check(lib.stair_plan_upload(res._plan, C.c_void_p(self._ws.data_ptr()), self._ws.numel() * 4,
                                        C.c_void_p(side.cuda_stream)))
            self._enqueue(side)                       # warm-up outside the capture (lazy module loading, attributes)
        torch.cuda.current_stream(dev).wait_stream(side)
        torch.cuda.synchronize(dev)
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph):
            self._enqueue(torch.cuda.current_stream(dev))

    def _enqueue(self, stream):
        res = self.result
        video, bf16 = res._src.video_arg()      # NULL: a plan of cached encodings (the index image uploaded above names their rows)
        check(lib.stair_plan_run_flags(res._model._ctx, res._plan, video,
                                       C.c_void_p(res._question.data_ptr()), C.c_void_p(self._ws.data_ptr()),
                                       self._ws.numel() * 4, C.c_void_p(self.logits.data_ptr()),
                                       C.c_void_p(self.pred.data_ptr()), RUN_INDEX_RESIDENT | bf16,
                                       C.c_void_p(stream.cuda_stream)))

    def replay(self):
        self.graph.replay()
        return self.logits, self.pred


class VideoNMN(nn.Module):
    def __init__(self, config, debug=False, pretrain_modules=set()):
        super().__init__()
        self.debug = debug
        self.config = dict(config)
        self.pretrain_modules = pretrain_modules
        self.contrastive_head = L2Normalize()
        self.words_to_keep = set(spec.KEYWORDS)

        self.submodules = nn.ModuleDict()
        for name in spec.MODULE_NAMES:
            self.submodules[name] = _TemporalNode() if name == 'Temporal' else _Node()
        for name in ('video_encoder', 'text_encoder', 'decoder'):
            self.submodules[name] = _Node()
        for key in spec.state_dict_keys(self.config):
            parts = key.split('.')[1:]                  # drop 'submodules'
            node = self.submodules[parts[0]]
            for part in parts[1:-1]:
                if part not in node._modules:
                    if parts[0] == 'Superlative' and part == 'localize_module':
                        node.add_module(part, self.submodules['Localize'])      # module_net.py:31-32
                    else:
                        node.add_module(part, _Node())
                node = node._modules[part]
            if parts[-1] not in node._parameters:
                shape = dict(spec.weight_table(self.config))[key]
                p = nn.Parameter(torch.empty(*shape))
                _init_param(key, p, self.config)
                node.register_parameter(parts[-1], p)
        if self.config['have_pretrain_head']:
            for name in ('Filter', 'Superlative', 'ToAction'):
                self.submodules[name].pretrain_head = self.contrastive_head     # modules.py:110,234,363
            for name in ('Localize', 'HasItem', 'ExistsFrame'):
                self.submodules[name].pretrain_head = nn.Identity()

        cfg = StairConfig(self.config['hidden_size'], self.config['video_size'], self.config['text_size'],
                          self.config['answer_vocab_length'], self.config['max_video_length'],
                          self.config['object_types'], 1 if self.config['have_pretrain_head'] else 0)
        handle = C.c_void_p()
        check(lib.stair_ctx_create(C.byref(cfg), C.byref(handle)))
        self._ctx = handle
        self._weight_names = [lib.stair_weight_name(self._ctx, i).decode() for i in range(lib.stair_weight_count(self._ctx))]
        self._bound = {}
        self._gbound = {}
        self._trainable = [True] * len(self._weight_names)      # what the context holds (stair_ctx_set_trainable; its default is 1)
        self._ws = None
        self._proj = None
        self._index_ring = None             # page-locked staging of the row numbers of library / word-table passes (made on first use)
        # run_programs: enqueue the encoders' input projections before the plan is built (False: inside the plan's pass)
        self.early_projection = True
        self._programs = frontend.ProgramCache()

    def __del__(self):
        ctx = self.__dict__.get('_ctx')
        if ctx:
            lib.stair_ctx_destroy(ctx)
            self.__dict__['_ctx'] = None        # plain dict write: nn.Module.__setattr__ may be gone at shutdown

    OPTIONS = {'matmul_mode': 0, 'tile_mlp': 1, 'tile_queue': 2, 'vec_group': 3, 'tn_slab_min_rows': 4}
    MATMUL_MODES = {'f32': 0, 'bf16x3': 1, 'bf16': 2}

    def set_option(self, name, value):
        """Per-context override of a process-wide library setting (stair_ctx_set_option): 'matmul_mode' ('f32' / 'bf16x3' / 'bf16'),
        'tile_mlp', 'tile_queue', 'vec_group' (0 / 1), 'tn_slab_min_rows', and 'tile_pack' (0 / 1: clips of at most 32 frames share
        a 64-row tile; stair_ctx_set_tile_pack) and 'tile_split' (0 / 1: clips of more than 64 frames run on the tile operators as
        64-row segments; stair_ctx_set_tile_split); None restores the process default.  In force for this
        model's forward and backward passes only: other models of the process keep their own settings."""
        if name == 'tile_pack':
            check(lib.stair_ctx_set_tile_pack(self._ctx, -1 if value is None else int(value)))
            return
        if name == 'tile_split':
            check(lib.stair_ctx_set_tile_split(self._ctx, -1 if value is None else int(value)))
            return
        if name == 'matmul_mode' and isinstance(value, str):
            value = self.MATMUL_MODES[value]
        check(lib.stair_ctx_set_option(self._ctx, self.OPTIONS[name], -1 if value is None else int(value)))

    # ---------------------------------------------------------------------------------------
    def _bind_weights(self):
        """(Re)hand the current parameter storage to the ctx; pointers are borrowed by the library."""
        sd = dict(self.named_parameters())
        for i, name in enumerate(self._weight_names):
            p = sd[name]
            if not p.is_cuda or p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError('parameter %s must be a contiguous float32 tensor on the GPU; call model.cuda()' % name)
            if self._bound.get(name) != p.data_ptr():
                check(lib.stair_ctx_set_weight(self._ctx, i, C.c_void_p(p.data_ptr()), p.numel()))
                self._bound[name] = p.data_ptr()

    def _sync_trainable(self):
        """requires_grad of every canonical weight -> the context, before every training pass: a frozen weight gets no gradient
        and no update, and the reverse pass launches nothing that only it needed (stair_ctx_set_trainable).  Only the bits that
        changed since the last pass cross the boundary.  Returns the flags in weight-table order."""
        sd = dict(self.named_parameters())
        for i, name in enumerate(self._weight_names):
            on = bool(sd[name].requires_grad)
            if self._trainable[i] != on:
                check(lib.stair_ctx_set_trainable(self._ctx, i, 1 if on else 0))
                self._trainable[i] = on
        return self._trainable

    def _bind_grads(self):
        sd = dict(self.named_parameters())
        trainable = self._sync_trainable()
        for i, name in enumerate(self._weight_names):
            if not trainable[i]:                 # frozen: the pass writes nothing for it, it needs no buffer
                continue
            g = sd[name].grad
            if g is None or not g.is_cuda or g.dtype != torch.float32 or not g.is_contiguous():
                raise RuntimeError('parameter %s has no contiguous float32 GPU .grad buffer; use stair_amd.train.Trainer '
                                   'or allocate p.grad = torch.zeros_like(p)' % name)
            if self._gbound.get(name) != g.data_ptr():
                check(lib.stair_ctx_set_grad(self._ctx, i, C.c_void_p(g.data_ptr()), g.numel()))
                self._gbound[name] = g.data_ptr()

    def _projection(self, nfloats, device):
        """The shared buffer of the encoders' input projections (same lifetime rules as the shared workspace: the next batch rewrites it)."""
        if self._proj is None or self._proj.numel() < nfloats or self._proj.device != device:
            self._proj = torch.empty(int(nfloats * 1.25), dtype=torch.float32, device=device)
        return self._proj

    def _workspace(self, nbytes, device):
        n = (nbytes + 3) // 4
        if self._ws is None or self._ws.numel() < n or self._ws.device != device:
            self._ws = torch.empty(int(n * 1.25), dtype=torch.float32, device=device)
        return self._ws

    # ---------------------------------------------------------------------------------------
    def _video_encoder_frozen(self):
        """The rule of training on encoded clips: all eight tensors of the video encoder have requires_grad = False."""
        sd = dict(self.named_parameters())
        return not any(sd[k].requires_grad for k in self._weight_names if '.video_encoder.' in k)

    def _check_mode(self, encoded, train, dropout):
        """The mode rules of a pass, applied before anything is built: training on encoded clips needs the video encoder frozen,
        dropout needs train=True."""
        if encoded and train and not self._video_encoder_frozen():
            raise ValueError('training on cached encodings needs a frozen video encoder: set requires_grad = False on all eight '
                             'submodules.video_encoder.* tensors (Trainer(freeze=(\'video_encoder\',))) -- the plan has no video encoder '
                             'to send gradients to, and a cache of a trainable one would be stale after the first step')
        if not train and dropout is not None and dropout[0] > 0:
            raise ValueError('dropout is a training-mode operation (train=True)' +
                             ('; this pass on cached clips is inference' if encoded else ''))

    def _clip_source(self, n, video, video_index, video_len, clips=None, encoded=None, train=False, dropout=None, library=None):
        """The ClipSource of a pass over n questions, one public form each: clips= (a ClipCache), encoded= (caller-made encodings),
        library= (a ClipLibrary of raw clip features), else video.  Checks everything that can be refused before a plan exists;
        enqueues nothing."""
        if library is not None:
            return self._source_of_library(n, library, video, video_index, video_len, clips, encoded, train, dropout)
        if clips is not None:
            return self._source_of_cache(n, clips, video, video_index, video_len, train, dropout)
        if encoded is not None:
            return self._source_of_encodings(n, encoded, video_index, video_len, train, dropout)
        return self._source_of_video(n, video, video_index, video_len, train, dropout)

    def _source_of_video(self, n, video, video_index, video_len, train, dropout):
        if video_index is not None:
            video_index = np.ascontiguousarray(np.asarray(video_index, dtype=np.int32))
            if video_index.shape != (n,):
                raise ValueError('video_index must have one entry per question')
            if video.dim() != 3 or n == 0 or video_index.min() < 0 or video_index.max() >= video.shape[0]:
                raise ValueError('video must be [n_videos, T, V] and video_index must point into it')
        elif video.dim() != 3 or video.shape[0] != n:
            raise ValueError('video must be [n, T, V]')
        # clip features: fp32, or the stored bf16 format of BASELINE.json configs[1] (video.dtype == torch.bfloat16): the
        # input projection of the video encoder then runs on the bf16 rows directly (two MFMA products per operand pair)
        ops._req(video, 'video', torch.bfloat16 if video.dtype == torch.bfloat16 else torch.float32)
        if video.dtype == torch.bfloat16 and self.config['video_size'] % 32:
            raise ValueError('bf16 clip features need video_size % 32 == 0')
        T = video.shape[1]
        if video_len is not None:
            video_len = np.ascontiguousarray(np.asarray(video_len, dtype=np.int32))
            if video_len.shape != (video.shape[0],):
                raise ValueError('video_len must have one entry per clip')
            if bool((video_len == T).all()):
                video_len = None
        self._check_mode(False, train, dropout)
        return ClipSource(video, None, None, None, video.shape[0], video_index, video_len, T)

    def _source_of_cache(self, n, clips, video, video_index, video_len, train, dropout):
        if video is not None or video_len is not None:
            raise ValueError('video given together with clips: a pass on cached clips takes video=None and no video_len (the cache '
                             'holds the encodings and their lengths)')
        self._check_mode(True, train, dropout)
        if video_index is None:
            raise ValueError('video_index is required with clips=: the cache row of every question\'s clip')
        clips.check()
        if clips.hidden_size != self.config['hidden_size'] or clips.device != next(self.parameters()).device:
            raise ValueError('the clip cache belongs to another configuration or device')
        return self._source_of_rows(clips.enc, clips, video_index, clips.lengths, n, 'the cache')

    def _source_of_encodings(self, n, encoded, video_index, video_len, train, dropout):
        self._check_mode(True, train, dropout)
        dev, H = next(self.parameters()).device, self.config['hidden_size']
        if not isinstance(encoded, torch.Tensor) or encoded.dim() != 3 or encoded.shape[2] != H or encoded.shape[0] == 0 or encoded.shape[1] == 0:
            raise ValueError('encoded must be a float32 [n_clips, T, %d] tensor of clip encodings, got shape %s'
                             % (H, tuple(getattr(encoded, 'shape', ()))))
        if encoded.device != dev or encoded.dtype != torch.float32 or not encoded.is_contiguous():
            raise ValueError('encoded must be a contiguous float32 tensor on the model\'s device %s' % (dev,))
        if encoded.shape[1] > self.config['max_video_length']:
            raise ValueError('encoded holds %d frames per clip, max_video_length is %d' % (encoded.shape[1], self.config['max_video_length']))
        n_clips, cap = encoded.shape[0], encoded.shape[1]
        if video_index is None:
            if n_clips != n:
                raise ValueError('video_index is required when encoded holds another number of clips than there are questions')
            video_index = np.arange(n, dtype=np.int32)
        lengths = np.full(n_clips, cap, np.int32) if video_len is None else np.ascontiguousarray(np.asarray(video_len, dtype=np.int32))
        if lengths.shape != (n_clips,) or lengths.min() < 1 or lengths.max() > cap:
            raise ValueError('video_len must hold the frames (1 .. %d) of each of the %d encoded clips' % (cap, n_clips))
        return self._source_of_rows(encoded, None, video_index, lengths, n, 'encoded')

    def _source_of_library(self, n, library, video, video_index, video_len, clips, encoded, train, dropout):
        """Clips named by ClipLibrary row: the plan's clips are the distinct rows in order of first use, as for a cache; the pass
        gathers them into a dense tensor (VideoNMN._gathered) and is from there on the pass of _source_of_video on that tensor."""
        if video is not None or clips is not None or encoded is not None:
            raise ValueError('library= given together with video=, clips= or encoded=: a pass on a clip library takes video=None and '
                             'names its clips by library row in video_index')
        if video_len is not None:
            raise ValueError('video_len= given together with library=: the library holds its clips\' lengths')
        if video_index is None:
            raise ValueError('video_index is required with library=: the library row of every question\'s clip')
        dev, V = next(self.parameters()).device, self.config['video_size']
        if library.device != dev or library.video_size != V:
            raise ValueError('library= belongs to another device or video_size: it holds %d features per frame on %s, the model reads '
                             '%d on %s' % (library.video_size, library.device, V, dev))
        if library.dtype == torch.bfloat16 and V % 32:
            raise ValueError('library= holds bf16 clip features, which need video_size % 32 == 0')
        used, index, lens, T = self._clips_of_rows(video_index, library.lengths, n, 'the library')
        if T > self.config['max_video_length'] or int(lens.max()) > self.config['max_video_length']:
            raise ValueError('library= holds a clip of %d frames among those asked for, max_video_length is %d'
                             % (int(lens.max()), self.config['max_video_length']))
        self._check_mode(False, train, dropout)
        return ClipSource(None, None, None, None, len(used), index, lens if bool((lens != T).any()) else None, T, library, used)

    def _gathered(self, src):
        """The source of a library pass once its clips are on their way: rows and lengths go up through a ring of page-locked buffers
        (no synchronise, no read-back) and one launch (stair_gather_clips) writes the dense [n_videos, T, V] tensor the encoder
        reads; the BatchResult keeps it (the reverse pass reads the clips again for dW_ih, an autograd call until backward())."""
        if src.library is None or src.video is not None:
            return src
        if self._index_ring is None:
            self._index_ring = _IndexRing()
        nv = src.n_videos
        host = src.library_rows if src.lens is None else np.concatenate([src.library_rows, src.lens])
        dev_idx = self._index_ring.upload(host, src.library.device)
        return src._replace(video=src.library.gather(dev_idx[:nv], dev_idx[nv:] if src.lens is not None else None, src.T))

    def _question_rows(self, question, question_ids, words, q_lens):
        """The question rows of a pass: `question` itself, or with question_ids= (host int32 [sum(q_lens)], rows of the WordTable
        `words`) the rows one launch gathers from the table (stair_gather_words).  Refusals come first; then the ids are uploaded
        and the gather enqueued."""
        if question_ids is None:
            if words is not None:
                raise ValueError('words= given without question_ids=: the table is read through the ids')
            return question
        if question is not None:
            raise ValueError('question_ids= given together with question=: a pass on a word table takes question=None')
        if words is None:
            raise ValueError('question_ids= needs words=: the WordTable the ids are rows of')
        dev, E = next(self.parameters()).device, self.config['text_size']
        if words.device != dev or words.dim != E:
            raise ValueError('words= belongs to another device or text_size: it holds %d floats per word on %s, the model reads %d on %s'
                             % (words.dim, words.device, E, dev))
        ids = words.check_ids(question_ids, int(sum(q_lens)))
        if self._index_ring is None:
            self._index_ring = _IndexRing()
        return words.gather(self._index_ring.upload(ids, dev))

    def _source_of_rows(self, enc, cache, video_index, lengths, n, what):
        used, index, lens, T = self._clips_of_rows(video_index, lengths, n, what)
        return ClipSource(None, enc, cache, used, len(used), index, lens if bool((lens != T).any()) else None, T)

    def _clips_of_rows(self, video_index, lengths, n, what):
        """(rows of the plan's clips, clip of every question, the clips' frames, T) for questions that name rows of `what`."""
        rows = np.ascontiguousarray(np.asarray(video_index, dtype=np.int32))
        if rows.shape != (n,) or n == 0 or rows.min() < 0 or rows.max() >= len(lengths):
            raise ValueError('video_index must hold one row of %s (0 .. %d) per question' % (what, len(lengths) - 1))
        # every distinct row is ONE clip of the plan (order of first use), so that questions about one clip share its nodes
        uniq, first, index = np.unique(rows, return_index=True, return_inverse=True)
        order = np.argsort(first, kind='stable')
        rank = np.empty_like(order)
        rank[order] = np.arange(len(order))
        used = np.ascontiguousarray(uniq[order].astype(np.int32))
        index = np.ascontiguousarray(rank[index].astype(np.int32))
        lens = np.ascontiguousarray(np.asarray(lengths, dtype=np.int32)[used])
        T = int(lens.max())
        if self.config['max_video_length'] <= 32:       # Linear(T,T) Temporal nets fix T (modules.py:266-277): the reference crashes on any other clip
            T = self.config['max_video_length']
            if bool((lens != T).any()):
                raise ValueError('Linear-Temporal configurations (max_video_length <= 32) need every clip at max_video_length = %d frames' % T)
        return used, index, lens, T

    def run_programs(self, programs, spans, video, question, q_lens, train=False, video_index=None, dropout=None, video_len=None,
                     before_run=None, cse=True, clips=None, library=None, question_ids=None, words=None):
        """Batched pass.  programs: list of token lists; spans: list of {pos: (lo, hi)}; video
        [n,T,V] and question [sum(q_lens), E] float32 on the GPU.  Returns a BatchResult.

        dropout (optional, training plans only): (p, seed) applies nn.Dropout(p) at the reference's positions with
        masks derived from `seed` (stair_plan_set_dropout); None or p = 0 is the eval / dropout=0 arithmetic that every
        parity test pins.
        video_index (optional, [n] ints): question q asks about clip video[video_index[q]]; video is then
        [n_videos,T,V] and each clip is encoded once instead of once per question (module_net.py:74 encodes per
        question; the results are identical).
        video_len (optional, [n_videos] ints): clips of different frame counts in one batch -- clip v holds video_len[v]
        <= T frames at the front of video[v], ZERO (at least finite) padding behind -- data.pack_questions and forward_batch
        pad with zeros; the padded rows take part in the weight-gradient products with zero coefficients, so NaN / Inf there
        would poison dW_ih (dataset.py:137-143 keeps every clip's own length); each
        question is computed as the reference computes a clip of its own length (stair_plan_build_ragged).
        cse: share common subexpressions across the batch (include/stair_hip.h STAIR_PLAN_NO_CSE): a node that depends only on
        the clip, keyword strings and identical question spans is computed once and aliased by every other occurrence; the
        values are those of the expanded computation (module_net.py:100-106), gradients of all users accumulate.  Ignored when
        dropout is active: the reference draws one mask per question and occurrence, a shared node would be dropped once for all.
        before_run (optional): called with the BatchResult after the plan is built (node table, slots and offsets are
        known) and BEFORE the pass is enqueued -- host work that only needs the plan (the loss driver's index arrays)
        then overlaps the previous step's GPU work instead of sitting between this step's forward and backward.
        clips (optional, a ClipCache of encode_clips): the clips were encoded before.  video is None, video_index [n] (required)
        names the CACHE ROW of every question's clip, in any order and with repeats; every distinct row becomes one clip of the
        plan (BatchResult.clip_rows), which runs no video encoder: one launch copies the cached rows into the map arena
        (STAIR_PLAN_VIDEO_ENCODED).  The plan's T is the longest clip used (max_video_length for the Linear-Temporal
        configurations, which admit no other length).  train=True (with dropout=, before_run= as on clips) is admitted while
        all eight tensors of the video encoder are frozen (requires_grad = False) and raises ValueError otherwise: the training
        plan keeps none of the encoder's saves, the reverse pass is the frozen-encoder pass, the encoder's tensors report
        untouched and the cache stays fresh.  dropout with train=False raises ValueError, and so does a cache whose encoder
        weights or matmul mode are no longer the model's (ClipCache.check).
        library (optional, a ClipLibrary: raw clip features kept on the device): video is None, video_index [n] (required) names
        the LIBRARY ROW of every question's clip, in any order and with repeats; every distinct row becomes one clip of the plan, in
        order of first use.  One launch (stair_gather_clips) writes the plan's clips, with their own lengths, into a dense tensor
        that the BatchResult keeps; from there the pass -- and, with train=True, the reverse pass of a TRAINABLE video encoder --
        is the one on `video`, the same launches on the same bytes.  The step uploads the rows and lengths only.  ValueError before
        anything is enqueued: library= with video=, clips=, encoded= or video_len=; a library on another device or of another
        video_size; bf16 features with video_size % 32 != 0; a clip longer than max_video_length.
        question_ids (optional, int32 [sum(q_lens)] on the HOST) with words (a data.WordTable) and question=None: the question rows
        are gathered on the device from the table's rows (stair_gather_words), bit for bit the rows embed_sent makes.  ValueError:
        question_ids= with question=, or without words=; an id outside the table."""
        src = self._clip_source(len(programs), video, video_index, video_len, clips, None, train, dropout, library)
        question = self._question_rows(question, question_ids, words, q_lens)
        return self._run(src, programs, spans, question, q_lens, train, dropout, before_run, cse)

    def _run(self, src, programs, spans, question, q_lens, train, dropout, before_run, cse):
        """The batched pass, once for every ClipSource (arguments as for run_programs).  What the forms differ in is read off `src`:
        the video arguments of the early projection, the clips of the build, the gather's operands, the video argument of the run."""
        n, dev, A = len(programs), question.device, self.config['answer_vocab_length']
        ops._req(question, 'question')
        self._bind_weights()
        if train:
            self._sync_trainable()              # (the builder, BatchResult.touched() and the reverse pass go by the context's flags)
        # under dropout every occurrence of a node draws its own mask (module_net.py:100-106 in model.train()): nothing is shared
        drop_on = dropout is not None and dropout[0] > 0
        stream = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        ip = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32)) if a is not None else None
        src = self._gathered(src)               # a library pass: its clips' gather goes first, the rest is the pass on clip features
        video, bf16 = src.video_arg()
        # The encoders' input projections need the inputs only: enqueue them BEFORE packing the programs and building the plan (3-4 ms
        # of host work at 2048 questions), so the device is busy meanwhile (stair_encoders_project; results bit-identical).
        # Encoded clips: the text projection alone (n_videos = 0)
        proj = None
        if self.early_projection and n > 0 and question.shape[0] > 0:
            nv = src.n_videos if src.video is not None else 0
            nf = int(lib.stair_projection_floats(self._ctx, nv, src.T, question.shape[0]))
            proj = self._projection(nf, dev)
            check(lib.stair_encoders_project(self._ctx, video, 1 if bf16 else 0, nv, src.T, C.c_void_p(question.data_ptr()),
                                             question.shape[0], C.c_void_p(proj.data_ptr()), proj.numel(), stream()))
        compiled = [self._programs.get(p, sp) for p, sp in zip(programs, spans)]       # packed once per distinct (program, spans)
        prog_off, tokens, lo, hi, q_off = frontend.pack_batch(compiled, q_lens)
        if question.shape[0] != int(q_off[-1]):
            raise ValueError('question rows (%d) != sum(q_lens) (%d)' % (question.shape[0], int(q_off[-1])))
        plan = C.c_void_p()
        check(lib.stair_plan_build_ragged(self._ctx, n, ip(prog_off), ip(tokens), ip(lo), ip(hi), ip(q_off), src.n_videos, ip(src.index),
                                          ip(src.lens), src.T,
                                          (PLAN_VIDEO_ENCODED if src.enc is not None else 0) | (1 if train else 0) |
                                          (0 if cse and not drop_on else 2) | (PLAN_EXT_PROJECTION if proj is not None else 0), C.byref(plan)))
        try:
            info = PlanInfo()
            check(lib.stair_plan_get_info(plan, C.byref(info)))
            if drop_on:
                check(lib.stair_plan_set_dropout(plan, C.c_float(float(dropout[0])), C.c_uint64(int(dropout[1]) & (2 ** 64 - 1))))
            if src.enc is not None:
                enc = src.enc
                check(lib.stair_plan_set_encoded_video(plan, C.c_void_p(enc.data_ptr()), enc.shape[1] * enc.shape[2], enc.shape[1], ip(src.rows)))
            ws = self._workspace(info.workspace_bytes, dev)
            if proj is not None:
                check(lib.stair_plan_set_projection(self._ctx, plan, C.c_void_p(proj.data_ptr()), proj.numel()))
            logits = torch.empty(n, A, dtype=torch.float32, device=dev)
            pred = torch.empty(n, dtype=torch.int32, device=dev)
        except Exception:
            lib.stair_plan_destroy(plan)
            raise
        res = BatchResult(self, plan, info, ws, logits, pred, prog_off, programs, src, question, proj)     # owns the plan from here on
        if before_run is not None:
            before_run(res)
        check(lib.stair_plan_run_flags(self._ctx, plan, video, C.c_void_p(question.data_ptr()), C.c_void_p(ws.data_ptr()), ws.numel() * 4,
                                       C.c_void_p(logits.data_ptr()), C.c_void_p(pred.data_ptr()),
                                       bf16 | (RUN_PROJECTED if proj is not None else 0), stream()))
        if train:       # a training plan keeps its logits inside the workspace for the backward pass; hand the caller a copy
            res.logits = ws[info.logits_off: info.logits_off + n * A].view(n, A).clone()    # (n x A floats) that survives the next step
        return res

    def _matmul_mode_now(self):
        """The matmul mode this model's passes run in: the context's override, else the process-wide setting."""
        v = C.c_int32(-1)
        check(lib.stair_ctx_get_option(self._ctx, self.OPTIONS['matmul_mode'], C.byref(v)))
        mode = v.value if v.value >= 0 else lib.stair_get_matmul_mode()
        return {v: k for k, v in self.MATMUL_MODES.items()}[mode]

    def _clip_stamp(self):
        """(matmul mode, state of the video-encoder weights): storage address and torch version counter of each tensor.  Every write
        torch knows of moves a counter -- load_state_dict, an optimizer step, an in-place update under no_grad -- and Trainer.step
        reports its native Adam update to the counters (torch.autograd.graph.increment_version); writes through `.data` or a raw
        pointer do not."""
        sd = dict(self.named_parameters())
        return self._matmul_mode_now(), tuple((sd[k].data_ptr(), sd[k]._version) for k in self._weight_names if '.video_encoder.' in k)

    def _encode_chunk(self, video, lens, out):
        """stair_encode_clips of one padded chunk [n, T, V] (fp32 or bf16, on the device) into out = [n, rows_cap, H] cache rows."""
        ops._req(video, 'video', torch.bfloat16 if video.dtype == torch.bfloat16 else torch.float32)
        n, T, V = video.shape
        if V != self.config['video_size']:
            raise ValueError('clips must have video_size = %d features per frame' % self.config['video_size'])
        if video.dtype == torch.bfloat16 and V % 32:
            raise ValueError('bf16 clip features need video_size % 32 == 0')
        self._bind_weights()
        nbytes = int(lib.stair_encode_clips_ws_bytes(self._ctx, n, T, out.shape[1]))
        if nbytes < 0:
            raise ValueError('chunk of %d clips x %d frames is too large for one call: lower batch_size' % (n, T))
        ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=video.device)
        dlen = None if bool((lens == T).all()) else torch.from_numpy(lens).to(video.device)
        check(lib.stair_encode_clips(self._ctx, C.c_void_p(video.data_ptr()), 1 if video.dtype == torch.bfloat16 else 0, n, T,
                                     C.c_void_p(dlen.data_ptr() if dlen is not None else None), C.c_void_p(out.data_ptr()), out.shape[1],
                                     C.c_void_p(ws.data_ptr()), ws.numel() * 4, C.c_void_p(torch.cuda.current_stream().cuda_stream)))
        if int(ws[:1].view(torch.int32).item()) != 0:      # the call's status word (one read-back per chunk of a one-time job)
            raise StairError('a cooperative LSTM hand-off timed out while encoding clips (its workgroups were not co-resident: another '
                             'queue on this GPU?); the encodings of this chunk hold NaN.  STAIR_LSTM_COOP=0 selects the one-workgroup kernels')

    def encode_clips(self, clips=None, ids=None, video_len=None, batch_size=1024, library=None):
        """Run the video encoder once over a library of clips and keep the result: a ClipCache (stair_amd/clip_cache.py) for
        run_programs(clips=...), forward_batch(clip_cache=...) and the evaluate drivers.  clips: a list of [L_i, V] tensors, or
        a padded [N, T, V] tensor with video_len; fp32, or bf16 (the stored clip-feature format).  ids: one hashable per clip
        (forward_batch looks clips up by the questions' 'video_id'); default: the row numbers.  The encodings are those a plan's
        own encoder pass computes (stair_encode_clips: the same kernels, in this model's matmul mode), [N, max_video_length, H]
        fp32 with zeros behind each clip's frames.  cache.add(...) appends more clips later.
        library (a ClipLibrary, with clips=None): the clips are the library's, read where they lie on the device -- no clip bytes
        cross from the host.  ids: the library ids to encode, in that order (default: all, in row order); they are the cache's ids."""
        from .clip_cache import ClipCache
        dev = next(self.parameters()).device
        if library is not None:
            if clips is not None or video_len is not None:
                raise ValueError('library= given together with clips= or video_len=: the library holds the clips and their lengths')
            if library.device != dev or library.video_size != self.config['video_size']:
                raise ValueError('library= belongs to another device or video_size')
            if ids is None:
                ids, clips, video_len = library.ids, library.clips, library.lengths
            else:
                ids = list(ids)
                rows = library.rows(ids)
                video_len = library.lengths[rows]
                clips = library.gather(torch.from_numpy(rows).to(dev), torch.from_numpy(video_len).to(dev), int(video_len.max()))
        elif clips is None:
            raise ValueError('encode_clips needs clips= or library=')
        cache = ClipCache(self.config['max_video_length'], self.config['hidden_size'], self._encode_chunk, self._clip_stamp, dev)
        cache.add(clips, ids=ids, video_len=video_len, batch_size=batch_size)
        return cache

    def logits(self, programs, spans, video, question, q_lens, video_index=None, video_len=None, dropout=None, cse=True, clips=None,
               encoded=None, library=None, question_ids=None, words=None):
        """[n, A] logits of a batch (arguments as for run_programs) with a torch autograd graph: when grad mode is on and any
        parameter, `video` or `question` requires grad, the result has a grad_fn whose backward runs the native reverse pass
        seeded by the logits gradient (stair_amd.autograd.PlanLogits) -- parameter gradients, and input gradients for `video`
        (fp32 or bf16) / `question` when they require grad.  A batch goes backward once; double backward is not supported.
        Otherwise an inference plan runs (dropout does not apply there) and the logits are those of run_programs.

        On encoded clips (video=None; the differentiable forms need the video encoder frozen, ValueError otherwise):
        clips=cache, video_index = the cache row of every question's clip -- autograd over a ClipCache; no gradient goes to the cache.
        encoded=enc, a float32 [n_clips, T, H] tensor on the GPU (the output of a clip encoder of the caller's own, in torch),
        video_index [n] (optional when n_clips == n) = the clip of every question, video_len [n_clips] (optional) = the clips'
        frames.  When enc requires grad it receives a gradient of its own shape: a clip's gradient is summed over the questions
        that share it, zero behind its video_len and zero for clips that no question reads.

        library=lib (a ClipLibrary, video=None, video_index = the library row of every question's clip) and question_ids= / words=
        are those of run_programs.  The video encoder may be trainable: its parameters receive their gradients as on `video`.  A
        library is data: no gradient goes to it, and a call that asks for the video's gradient has to hand the clips in as video=
        (a `video` tensor beside library= is refused like any other).  The gathered question rows receive no gradient either."""
        params = [dict(self.named_parameters())[n] for n in self._weight_names]
        if library is None and (clips is not None or encoded is not None) and (video is not None or (clips is not None and encoded is not None)):
            raise ValueError('video given together with clips= / encoded=: a pass on encoded clips takes video=None and one of the two')
        if library is not None and isinstance(video, torch.Tensor) and video.requires_grad:
            raise ValueError('library= given together with a video= that requires grad: a library is data and receives no gradient; '
                             'the gradient of the video needs the clips handed in as video= alone')
        tensor = video if video is not None else encoded        # what of the source autograd may differentiate (a ClipCache: nothing)
        grad = torch.is_grad_enabled() and ((question is not None and question.requires_grad) or any(p.requires_grad for p in params) or
                                            (isinstance(tensor, torch.Tensor) and tensor.requires_grad))
        src = self._clip_source(len(programs), video, video_index, video_len, clips, encoded, grad, dropout if grad else None, library)
        question = self._question_rows(question, question_ids, words, q_lens)
        if not grad:
            with torch.no_grad():
                return self._run(src if tensor is None else src.with_tensor(tensor.detach()), programs, spans, question, q_lens,
                                 False, None, None, cse).logits
        from .autograd import PlanLogits
        return PlanLogits.apply(self, (programs, spans, q_lens, dropout, cse, src), tensor, question, *params)

    def forward_batch(self, batch, train=False, share_videos=True, dropout=None, cse=True, clip_cache=None, clip_library=None):
        """batch: list of question dicts in the reference layout (dataset.py:191-233).  Clips may differ in their
        number of frames (they are padded to the longest of the batch and run with their own lengths, see run_programs);
        Linear-Temporal configurations (max_video_length <= 32) need every clip at max_video_length, like the reference.
        Tensors may live on the host; they are moved once, packed.

        Questions about the same clip share one encoder pass.  AGQADataset hands every question of a video the
        same `self.video_feats[video_id]` tensor (dataset.py:183), so clips are told apart by the memory their
        `video_features` occupy (or by a `video_id` entry, when every dict carries one).

        clip_cache (a ClipCache of encode_clips): the clips are looked up by d['video_id'] and not encoded again (their
        'video_features' are not read); an id the cache does not hold raises KeyError naming it.  With train=True the video
        encoder must be frozen (see run_programs, `clips`).
        clip_library (a ClipLibrary): the clips are looked up by d['video_id'] in the library and gathered on the device (their
        'video_features' are not read, nothing of them is copied from the host); a missing id raises KeyError naming it."""
        dev = next(self.parameters()).device
        video = video_len = None
        if clip_cache is not None and clip_library is not None:
            raise ValueError('clip_cache= given together with clip_library=: one source of clips per pass')
        if clip_cache is not None or clip_library is not None:
            index = (clip_cache if clip_cache is not None else clip_library).rows([d['video_id'] for d in batch])
        else:
            video, index, video_len = self._pack_clips(batch, share_videos, dev)
        qs = [torch.as_tensor(d['question']) for d in batch]
        question = torch.cat(qs).to(dev, torch.float32).contiguous()
        return self.run_programs([d['nmn_program_list'] for d in batch], [d['prog_str_to_question_tokens'] for d in batch], video, question,
                                 [q.shape[0] for q in qs], train=train, video_index=index, dropout=dropout, video_len=video_len, cse=cse,
                                 clips=clip_cache, library=clip_library)

    @staticmethod
    def _pack_clips(batch, share_videos, dev):
        """(video [n_videos, T, V] on the device, clip of every question or None, frames of every clip or None) of a batch of dicts."""
        clips, index = [], None
        if share_videos and len(batch) > 1:
            by_id = all('video_id' in d for d in batch)
            seen, index = {}, []
            for d in batch:
                key = d['video_id'] if by_id else _clip_key(d['video_features'])
                if key not in seen:
                    seen[key] = len(clips)
                    clips.append(d['video_features'])
                index.append(seen[key])
            if len(clips) == len(batch):
                index = None
        else:
            clips = [d['video_features'] for d in batch]
        clips = [torch.as_tensor(c) for c in clips]
        # clips stored as bf16 (data.load_clip_features(..., dtype='bf16')) stay bf16 on the device
        vdtype = torch.bfloat16 if all(c.dtype == torch.bfloat16 for c in clips) else torch.float32
        frames = [int(c.shape[0]) for c in clips]
        video_len = None
        if len(set(frames)) > 1:                   # mixed clip lengths: pad to the longest, keep every clip's own length
            video_len, Tm = frames, max(frames)
            clips = [torch.nn.functional.pad(c.to(vdtype), (0, 0, 0, Tm - c.shape[0])) for c in clips]
        return torch.stack(clips).to(dev, vdtype).contiguous(), index, video_len

    # ---------------------------------------------------------------------------------------
    @torch.no_grad()
    def forward(self, data, return_res_by_step=True, return_result_of_each_step=False, test_mode=False):
        """Single-question form with the reference's return dict (module_net.py:65-145)."""
        program_list, program_idx = data['nmn_program_list'], data['nmn_program_idx']
        res = self.forward_batch([data])
        heads = self.config['have_pretrain_head']

        new_sg_res_by_step = dict()
        if not test_mode:
            for key, value in data.get('sg_res_by_step', {}).items():      # module_net.py:78-89
                if isinstance(value, list) and len(value) and isinstance(value[0][1], torch.Tensor):
                    ans = []
                    for v_class_name, v_emb in value:
                        _, v_emb = self.encode_question_no_grad(v_emb)
                        ans.append((v_class_name, self.contrastive_head(v_emb)))
                    new_sg_res_by_step[key] = ans
                else:
                    new_sg_res_by_step[key] = value

        res_by_step, each = dict(), []
        arity = spec.ARITY
        if return_res_by_step or return_result_of_each_step:
            values = [res.node(0, i) for i in range(len(program_list))]
            values = [v.clone() if isinstance(v, torch.Tensor) else v for v in values]
            # children of each module token, in pop order (module_net.py:100-106)
            stack, children = [], [None] * len(program_list)
            for i in range(len(program_list) - 1, -1, -1):
                if program_list[i] in arity:
                    children[i] = [stack.pop() for _ in range(arity[program_list[i]])]
                stack.append(i)
            for i in range(len(program_list) - 1, -1, -1):
                prog = program_list[i]
                if prog in arity:
                    result = values[i]
                    if prog == 'Temporal':
                        self.submodules['Temporal'].related_attn = res.related_attn(0, i).clone()
                    if return_res_by_step and program_idx[i] is not None and prog in self.pretrain_modules and i != 0:
                        out = self.submodules[prog].pretrain_head(result) if heads else result
                        res_by_step[program_idx[i]] = (prog, out)
                    if return_result_of_each_step:
                        params = [values[c] for c in children[i]]
                        if heads and prog in self.pretrain_modules:
                            each.append((params, self.submodules[prog].pretrain_head(result)))
                        else:
                            each.append((params, result))
                elif return_result_of_each_step:
                    each.append(([], values[i]))

        ret = {'logits': res.logits[0], 'res_by_step': res_by_step}
        if return_result_of_each_step:
            ret['result_of_each_step'] = list(reversed(each))
        if not test_mode:
            ret['sg_res_by_step'] = new_sg_res_by_step
        return ret

    @torch.no_grad()
    def encode_question_no_grad(self, question):
        return self.encode_question(question)

    def _lstm_weights(self, enc):
        m = self.submodules[enc]
        return [getattr(m, n + sfx) for sfx in ('', '_reverse')
                for n in ('weight_ih_l0', 'weight_hh_l0', 'bias_ih_l0', 'bias_hh_l0')]

    def encode_question(self, question):
        """module_net.py:151-158 -> (token_feature [Q,H], sentence feature [H])."""
        dev = next(self.parameters()).device
        x = torch.as_tensor(question).to(dev, torch.float32).contiguous()
        off = torch.tensor([0, x.shape[0]], dtype=torch.int32, device=dev)
        out, h_n = ops.lstm_bidir(x, off, x.shape[0], self._lstm_weights('text_encoder'))
        return out, h_n[0]

    @torch.no_grad()
    def encode_phrases(self, phrase_embeddings):
        """Batched form of evaluate.py:66-76 (get_kw_representations): every phrase [L_i, E] through the text
        encoder in one ragged pass, sentence feature -> contrastive_head.  Returns [C, H] L2-normalised reps."""
        dev = next(self.parameters()).device
        xs = [torch.as_tensor(p).to(dev, torch.float32).reshape(-1, self.config['text_size']) for p in phrase_embeddings]
        lens = [int(x.shape[0]) for x in xs]
        if not xs or min(lens) <= 0:
            raise ValueError('every phrase needs at least one word embedding')
        off = torch.tensor(np.concatenate([[0], np.cumsum(lens)]), dtype=torch.int32, device=dev)
        _, h_n = ops.lstm_bidir(torch.cat(xs).contiguous(), off, max(lens), self._lstm_weights('text_encoder'))
        return ops.l2normalize(h_n)

    def encode_video(self, video_feat):
        """module_net.py:160-163 -> [T,H]."""
        dev = next(self.parameters()).device
        x = torch.as_tensor(video_feat).to(dev, torch.float32).contiguous()
        off = torch.tensor([0, x.shape[0]], dtype=torch.int32, device=dev)
        out, _ = ops.lstm_bidir(x, off, x.shape[0], self._lstm_weights('video_encoder'))
        return out
