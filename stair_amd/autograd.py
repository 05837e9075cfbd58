"""Torch autograd for ``VideoNMN``'s logits: the native reverse pass (csrc/plan.hip) seeded by whatever gradient autograd hands it.

``VideoNMN.logits(...)`` applies ``PlanLogits``: the forward pass runs a training plan on buffers of its own, and the backward pass
calls ``stair_plan_backward_dlogits`` with the incoming logits gradient -- any loss on the logits works (label smoothing, class
weights, distillation), and ``video`` / ``question`` receive input gradients when they require them (a trainable adapter in front of
the executor, frame- or word-level saliency).  What the reference does with ``batch_loss.backward()`` (train_module.py:408).

Semantics:

* the parameters are INPUTS of the Function: their gradients go back through autograd, so ``torch.autograd.grad``, hooks and
  ``.grad`` accumulation over several ``backward()`` calls behave as for any module.  Parameters that no program of the batch uses
  (``stair_plan_touched``) get ``None``, as unused modules do in the reference (train_module.py:408-410), and so do parameters
  with ``requires_grad = False``: the forward call hands the flags to the context (``VideoNMN._sync_trainable``), and the reverse
  pass then launches nothing that only they needed -- a frozen encoder costs no BPTT unless ``video`` / ``question`` asks for its
  input gradient;
* on encoded clips (a ``ClipCache``, or the caller's own encodings) the video encoder must be frozen; the encodings' gradient is the
  adjoint of the plan's gather (``stair_plan_set_encoded_video_grad``): summed over the questions that share a clip, zero behind a
  clip's frames and for clips that no question reads;
* every differentiable call owns its workspace and projection buffer until its backward has run (the model's shared buffers are
  rewritten by the next batch), so several outstanding forwards may go backward together; the buffers are released afterwards;
* a batch goes backward ONCE: BPTT overwrites the saved gates with their gradients.  A second backward through the same logits
  raises, with or without ``retain_graph=True``;
* double backward is not supported (``once_differentiable``).
"""
from __future__ import annotations

import ctypes as C

import torch
from torch.autograd.function import once_differentiable

from ._lib import check, lib

_SEG = 64          # gradient buffers start on 256-byte boundaries inside one flat allocation


class PlanLogits(torch.autograd.Function):
    """apply(model, call, video, question, *params) -> logits [n, A]; `call` = (programs, spans, q_lens, dropout, cse, src) as for
    ``VideoNMN.run_programs``, src the pass's ``ClipSource``; `params` in the order of ``model._weight_names``.  `video` is the
    tensor of the source that autograd sees: the clip features, or on encoded clips (``VideoNMN.logits(clips=...)`` /
    ``(encoded=...)``) None (a ClipCache: no gradient goes to it) or the encodings [n_clips, T, H], whose gradient comes back in
    their shape."""

    @staticmethod
    def forward(ctx, model, call, video, question, *params):
        programs, spans, q_lens, dropout, cse, src = call
        if video is not None:
            src = src.with_tensor(video.detach())
        shared = model._ws, model._proj
        model._ws = model._proj = None           # the pass allocates buffers for THIS batch; the shared ones are put back
        try:
            res = model._run(src, programs, spans, question.detach(), q_lens, True, dropout, None, cse)
        finally:
            model._ws, model._proj = shared
        ctx.model, ctx.res = model, res
        ctx.video_dtype = video.dtype if video is not None else None
        ctx.encoded = src.enc is not None        # (a ClipLibrary pass has neither tensor here: its clips are gathered inside the pass)
        return res.logits

    @staticmethod
    @once_differentiable
    def backward(ctx, d_logits):
        res = ctx.res
        if res is None:
            raise RuntimeError('VideoNMN.logits: this batch has been through backward() already -- its reverse pass overwrote the '
                               'saved LSTM gates with their gradients, so it cannot go backward again (retain_graph does not change '
                               'that); run model.logits(...) again')
        ctx.res = None
        model = ctx.model
        params = dict(model.named_parameters())
        names = model._weight_names
        need_p = ctx.needs_input_grad[4:]
        # a fresh zeroed gradient buffer per call: the pass ACCUMULATES into whatever is bound
        offs, total = [], 0
        for name in names:
            offs.append(total)
            total += (params[name].numel() + _SEG - 1) // _SEG * _SEG
        dev = res.logits.device
        flat = torch.zeros(total, dtype=torch.float32, device=dev)
        grads = [flat[o: o + params[name].numel()].view_as(params[name]) for o, name in zip(offs, names)]
        # (encoded clips: the pass stores the rows of the plan's clips only -- clips that no question reads keep these zeros)
        d_encoded = torch.zeros(res._enc.shape, dtype=torch.float32, device=dev) if ctx.encoded and ctx.needs_input_grad[2] else None
        d_video = torch.empty(res._video.shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[2] and not ctx.encoded else None
        d_question = torch.empty(res._question.shape, dtype=torch.float32, device=dev) if ctx.needs_input_grad[3] else None
        try:
            for i, g in enumerate(grads):
                check(lib.stair_ctx_set_grad(model._ctx, i, C.c_void_p(g.data_ptr()), g.numel()))
            res.backward_dlogits(d_logits.detach().to(torch.float32).contiguous(), d_video, d_question, bind_grads=False,
                                 d_encoded=d_encoded)
            touched = res.touched()
        finally:
            model._gbound = {}                   # a Trainer (or BatchResult.backward) used later binds its own buffers again
            del res                              # the plan, its workspace and projection buffer go (stream-ordered reuse)
        if d_video is not None and ctx.video_dtype != torch.float32:
            d_video = d_video.to(ctx.video_dtype)
        if ctx.encoded:
            d_video = d_encoded
        out = [g if (t and need) else None for g, t, need in zip(grads, touched, need_p)]
        return (None, None, d_video, d_question, *out)
