"""Training driver: the batched, data-parallel counterpart of the reference's loop
(/root/reference/train_module.py:341-412) for the decoder-loss configuration (module_loss_weight = 0):

    for each window of `global_batch` questions:        # the reference: gradient_accumulation = 32, batch 1
        loss = sum_i CE(logits_i, answer_i) * decoder_loss_weight / global_batch      (:376-380, :372)
        loss.backward(); Adam.step(); zero_grad(); LambdaLR.step()                     (:408-412)

One window = one batched forward + one HIP backward pass per rank (questions sharded across ranks);
gradients live in ONE flat fp32 buffer that is sum-reduced over RCCL once per step.  The buffer is laid out
`[module + decoder gradients | encoder gradients | touched mask | status word]`:

* the per-parameter "touched" mask rides behind the gradients (a parameter is touched if ANY rank's shard used
  its module), so that parameters of modules no rank used are skipped by Adam exactly as torch skips grad == None;
* the plan's status word (a cooperative recurrence that timed out: NaN gradients) rides there too, so the reduced
  word is the SAME on every rank: Adam's guard and Trainer.check() read it, and either every rank applies the
  step or none does (a failure local to one rank would otherwise poison the replicas through the sum and then
  leave its peers waiting in the next collective);
* with `overlap_allreduce` (default at world > 1) the bucket goes in two pieces: the module + decoder part -- final
  when the last program level's backward returns (stair_plan_set_backward_event) -- is reduced on a side stream
  while BPTT and the encoders' dW_ih / dW_hh products still run; `[encoder gradients | mask | status]` follows on
  the main stream.  Sums of two ranks are bit-identical to the one-piece reduction.

Parameters, gradients and Adam moments are flat buffers whose per-tensor segments start on multiples of 256
floats; the model's Parameters are views into them.
"""
from __future__ import annotations

import ctypes as C

import torch

from ._lib import check, lib

SEG = 256


def reduce_gradients(flat_g, touched, world, bucket=None, comm=None, status=None, split=None, side_stream=None, ready_event=None,
                     late_events=None):
    """The exchange step of data-parallel training: sum the flat fp32 gradient bucket over all ranks and OR the
    per-parameter touched mask (a parameter is "touched" if ANY rank's shard used its module).
    With `bucket` (a buffer whose head is flat_g and whose tail has room for the mask and one status word, as Trainer lays
    it out) the mask travels as floats behind the gradients and ONE all-reduce does both; without it, two collectives.
    status (optional, needs bucket): a one-element integer tensor, this rank's "the pass failed" word; it is summed in the
    word behind the mask and comes back as 1 on EVERY rank when any rank's was set.
    split (optional, needs bucket): the bucket goes as two collectives, bucket[:split] and bucket[split:] (the second holds
    mask and status).  On CUDA with side_stream + ready_event the first one is issued on side_stream once ready_event has
    fired -- beside whatever the current stream is still doing -- and the current stream waits for it at the end.
    late_events: an (e0, e1) pair of torch.cuda.Event(enable_timing=True) recorded on the current stream around the part of
    the exchange the current stream has to sit through (all of it in one-piece mode).
    Backend-agnostic (RCCL on GPUs, gloo in the CPU test); in place.  comm: a stair_amd.comm.NativeComm -- the bucket then
    goes through the C ABI's stair_allreduce_grads (RCCL from libstair_hip.so, same stream, no torch collective)."""
    if world <= 1:
        return flat_g, touched
    import torch.distributed as dist

    def allreduce(x):
        if comm is not None:
            comm.allreduce_(x)
        else:
            dist.all_reduce(x, op=dist.ReduceOp.SUM)

    if bucket is None:
        assert status is None and split is None
        dist.all_reduce(flat_g, op=dist.ReduceOp.SUM)
        dist.all_reduce(touched, op=dist.ReduceOp.MAX)
        return flat_g, touched
    n, k = flat_g.numel(), touched.numel()
    tail = bucket[n: n + k]
    tail.copy_(touched.to(bucket.dtype))
    if status is not None:
        bucket[n + k: n + k + 1].copy_((status != 0).to(bucket.dtype))
    if split is None:
        if late_events:
            late_events[0].record()
        allreduce(bucket)
    else:
        early, late = bucket[:split], bucket[split:]
        if side_stream is not None:
            with torch.cuda.stream(side_stream):
                if ready_event is not None:
                    side_stream.wait_event(ready_event)
                else:
                    side_stream.wait_stream(torch.cuda.current_stream())
                allreduce(early)
        else:
            allreduce(early)
        if late_events:
            late_events[0].record()
        allreduce(late)
        if side_stream is not None:
            torch.cuda.current_stream().wait_stream(side_stream)
    if late_events:
        late_events[1].record()
    touched.copy_((tail > 0).to(touched.dtype))
    if status is not None:
        status.copy_((bucket[n + k: n + k + 1] > 0).to(status.dtype))
    return flat_g, touched


class _PinnedRing:
    """Small host -> device uploads (the per-step touched mask) without tying the host to the stream: a pageable
    `.to(device)` makes the host wait until the stream has reached the copy -- the end of the backward pass -- and a single
    page-locked buffer has to wait for its previous copy, which is the same thing one step later.  A ring of `depth`
    page-locked buffers waits only for the copy issued `depth` steps ago, so the host may run that far ahead."""

    def __init__(self, numel, depth=8):
        self.bufs = [torch.empty(numel, dtype=torch.int32).pin_memory() for _ in range(depth)]
        self.events = [None] * depth
        self.i = 0

    def upload(self, values, device):
        k = self.i
        self.i = (k + 1) % len(self.bufs)
        if self.events[k] is not None:
            self.events[k].synchronize()
        self.bufs[k].copy_(torch.tensor(values, dtype=torch.int32))
        t = self.bufs[k].to(device, non_blocking=True)
        self.events[k] = torch.cuda.Event()
        self.events[k].record()
        return t


class Trainer:
    def __init__(self, model, lr=2e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoder_loss_weight=1.0,
                 module_loss_weight=1.0, contrastive_window=32, no_intermediate=('FilterFrame',),
                 scheduler_start_factor=1.0, scheduler_end_factor=0.1, scheduler_total_iters=200000, world=1,
                 skip_untouched='ever', train_module_before_iters=1e10, train_decoder_after_iters=0, rank=0,
                 dropout=None, dropout_seed=0, native_allreduce=False, class_table=None, global_batch=None, overlap_allreduce=None,
                 max_grad_norm=None, freeze=()):
        """freeze: name prefixes of parameters to freeze, in state_dict terms without the leading 'submodules.' -- a module or
                encoder ('video_encoder', 'Filter': not FilterFrame), a layer ('Filter.param.representation.0') or one tensor
                ('decoder.3.weight').  A convenience for p.requires_grad_(False): the flags themselves are read again at every
                step, so a schedule may thaw (or freeze) parameters between steps.  A frozen parameter gets no gradient (its
                p.grad segment stays zero), no update (weight, both moments and step count keep their bits), counts for nothing
                in grad_norm / the clip coefficient / seg_grad_norm (what clip_grad_norm_ does over parameters without a
                gradient), and the reverse pass launches nothing that only it needed (include/stair_hip.h,
                stair_ctx_set_trainable).  At world > 1 the frozen set must be the same on every rank; this is not checked.
        skip_untouched: 'ever'   -- a parameter is skipped by Adam until the first window that sends it a gradient
                                      (torch 1.13, which the reference pins: zero_grad() keeps zero tensors afterwards); a
                                      frozen parameter counts from the first step in which it is trainable AND used;
                           'window' -- skipped in every window that does not touch it (torch >= 2.0, set_to_none=True).
        max_grad_norm: None (default) -- the step is the reference's, which has no clipping: nothing extra is launched;
                       a positive float -- torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) between the gradient
                                      exchange and Adam, on the device (stair_grad_norm + stair_adam_step_scaled, no host
                                      read-back), and a step whose gradient norm is not finite is REFUSED: weights, moments
                                      and step counts stay those of the last good step and check() raises;
                       float('inf') -- measure and refuse non-finite steps, never scale (the coefficient is exactly 1).
                       The clip coefficient is applied inside the Adam kernel: `p.grad` (views of flat_g) keeps the UNCLIPPED
                       reduced gradient.  At world > 1 the norm is that of the summed bucket, the same bits on every rank, so
                       coefficient, decision and update are the same everywhere with no second collective.
                       Telemetry: grad_norm, seg_grad_norm, grad_norms_by_name(), finished_grad_norms()."""
        # train_module.py:350,376 gate the two loss families by the reference's global_steps (one per QUESTION there):
        # intermediate losses while global_steps < train_module_before_iters, decoder loss once global_steps >
        # train_decoder_after_iters.  Question i of a rank's shard has global step seen + 1 + rank + i * world.
        # class_table (losses.ClassTable, the same on every rank): the contrastive pools of a data-parallel step are then
        # exchanged as a [windows, classes] presence matrix summed on the device -- without it every supervised step at
        # world > 1 gathers the ranks' class lists through the host (all_gather_object), a blocking second collective.
        # global_batch: the window size summed over all ranks when it is the same every step (a data loader with drop_last).
        # Without it -- here or in step() -- every step at world > 1 agrees on the size with an extra all-reduce and a host
        # read-back (.item(): the host then waits for the stream, which ends its run-ahead); ragged last windows need that.
        # overlap_allreduce: None = on at world > 1; False = the whole bucket in ONE collective after the backward pass.
        self.global_batch = global_batch
        self.overlap_allreduce = (world > 1) if overlap_allreduce is None else bool(overlap_allreduce)
        self.inject_failure = False                          # test hook: set this rank's status word after the backward pass
        self.inject_nonfinite = False                        # test hook: +inf into this rank's first gradient element after the backward pass
        if max_grad_norm is not None:
            if isinstance(max_grad_norm, bool) or not isinstance(max_grad_norm, (int, float)) or not max_grad_norm > 0:
                raise ValueError('max_grad_norm must be None or a positive number (float("inf"): measure only), got %r' % (max_grad_norm,))
            max_grad_norm = float(max_grad_norm)
        self.max_grad_norm = max_grad_norm
        self.class_table = class_table
        self.allreduce_events = None                        # set to [] to collect (start, end) events around the step's collective
        self.before_iters, self.after_iters, self.rank = train_module_before_iters, train_decoder_after_iters, rank
        self.questions_seen = 0
        # nn.Dropout(config['dropout']) of the reference's model.train() (modules.py `D` positions, args.py:31).  Default:
        # the model's own config['dropout'], i.e. the reference's training recipe; the parity pins are defined at dropout = 0
        # (torch's Philox masks cannot be reproduced) and the tests / bench pass dropout=0.0 explicitly.
        # Every step and rank draws fresh masks: seed = dropout_seed + step * world + rank.
        self.dropout = float(model.config.get('dropout', 0.0) if dropout is None else dropout)
        self.dropout_seed = int(dropout_seed)
        assert skip_untouched in ('ever', 'window')
        self.skip_untouched = skip_untouched
        self.model, self.world = model, world
        self.lr, self.betas, self.eps, self.wd = lr, betas, eps, weight_decay
        self.decoder_loss_weight = decoder_loss_weight
        self.module_loss_weight, self.contrastive_window, self.no_intermediate = module_loss_weight, contrastive_window, no_intermediate
        self.sched = (scheduler_start_factor, scheduler_end_factor, scheduler_total_iters)
        self.iters = 0                                      # optimizer steps taken (LambdaLR counter)
        params = dict(model.named_parameters())
        names = model._weight_names
        freeze = (freeze,) if isinstance(freeze, str) else tuple(freeze)
        for pre in freeze:
            pre = pre[len('submodules.'):] if pre.startswith('submodules.') else pre
            hit = [nme for nme in names if nme[len('submodules.'):] == pre or nme[len('submodules.'):].startswith(pre + '.')]
            if not hit:
                raise ValueError('freeze: no parameter is named %r or lies under it' % pre)
            for nme in hit:
                params[nme].requires_grad_(False)
        dev = next(model.parameters()).device
        assert dev.type == 'cuda', 'Trainer needs the model on the GPU'
        # flat order: everything but the encoders first (their gradients are final before BPTT starts), the encoders last
        late = [i for i, nme in enumerate(names) if '_encoder.' in nme]
        order = [i for i in range(len(names)) if i not in set(late)] + late
        offs, total = [0] * len(names), 0
        self.split = None
        for i in order:
            if late and i == late[0]:
                self.split = total                           # bucket[:split] = module + decoder gradients, bucket[split:] = the rest
            offs[i] = total
            total += (params[names[i]].numel() + SEG - 1) // SEG * SEG
        self.n = total
        self.flat_p = torch.zeros(total, device=dev)
        mask_room = (len(names) + 1 + SEG - 1) // SEG * SEG   # touched mask as floats + the status word
        self.bucket = torch.zeros(total + mask_room, device=dev)       # [gradients | touched mask | status]
        self.flat_g = self.bucket[:total]
        self.exp_avg = torch.zeros(total, device=dev)
        self.exp_avg_sq = torch.zeros(total, device=dev)
        seg_of_block = torch.empty(total // SEG, dtype=torch.int32)
        for i, nme in enumerate(names):
            p = params[nme]
            view = self.flat_p[offs[i]: offs[i] + p.numel()].view_as(p)
            view.copy_(p.data)
            p.data = view                                    # Parameters become views of the flat buffer
            p.grad = self.flat_g[offs[i]: offs[i] + p.numel()].view_as(p)
            nb = (p.numel() + SEG - 1) // SEG
            seg_of_block[offs[i] // SEG: offs[i] // SEG + nb] = i
        self.seg_of_block = seg_of_block.to(dev)
        self._params = [params[nme] for nme in names]
        self.steps = torch.zeros(len(names), device=dev)     # per-tensor Adam step counts
        self.touched = torch.zeros(len(names), dtype=torch.int32, device=dev)
        self._ever = [False] * len(names)                    # host view of 'ever': touched in some step so far (on this rank)
        self._mask_ring = _PinnedRing(len(names))
        self._train_ring = _PinnedRing(len(names))           # the trainable flags of a step, uploaded only while something is frozen
        self._status = []                                    # (step, pinned int32 copy of the step's REDUCED status word, event) per step in flight
        self.guard = torch.zeros(1, dtype=torch.int32, device=dev)      # status of the current step, summed over ranks: Adam's guard
        self._side = self._ev_ready = None
        if self.overlap_allreduce and world > 1 and self.split:
            self._side = torch.cuda.Stream(device=dev)
            self._ev_ready = torch.cuda.Event()
            self._ev_ready.record()                          # creates the hipEvent_t the backward pass records (stair_plan_set_backward_event)
        self.allreduce_late_events = None                    # set to [] to collect (e0, e1) around the exposed part of the exchange
        self.comm = None
        if native_allreduce and world > 1:          # the step's one collective through the C ABI (stair_allreduce_grads)
            from .comm import NativeComm
            self.comm = NativeComm(rank, world)
        self.offsets = offs
        self.grad_norm = self.seg_grad_norm = None
        if max_grad_norm is not None:
            # [global L2 norm, clip coefficient] and the per-tensor norms (weight-table order) of the last step: device tensors,
            # written by the step's stair_grad_norm -- reading them synchronises, step() does not
            self.grad_norm = torch.zeros(2, device=dev)
            self.seg_grad_norm = torch.zeros(len(names), device=dev)
            self._seg_first_block = torch.tensor([o // SEG for o in offs], dtype=torch.int32, device=dev)
            self._seg_numel = torch.tensor([params[nme].numel() for nme in names], dtype=torch.int64, device=dev)
            self._norm_scratch = torch.empty(total // SEG, device=dev)
            self._norms = []                                 # (step, pinned copy of grad_norm, event) per step not yet handed out
            self._norm_free = []                             # pinned buffers to reuse

    def lr_factor(self):
        """train_module.py:328-331."""
        start, end, total = self.sched
        return end if self.iters > total else start + (end - start) / total * self.iters

    def step(self, programs, spans, video, question, q_lens, answers, global_batch=None, questions=None, video_index=None,
             video_len=None, clips=None, library=None, question_ids=None, words=None):
        """One optimizer step over this rank's shard of a window.  `questions` -- the dicts, with 'sg_res_by_step', or their
        losses.GoldBatch (losses.collate_gold: the data loader's collate step; the per-question bookkeeping then costs the stepping
        process nothing) -- switches the per-module intermediate losses on (train_module.py:351-373, 388-406).
        video_index: questions that share a clip (see VideoNMN.run_programs).
        clips (a ClipCache of VideoNMN.encode_clips, with video=None and video_index = the cache row of every question's clip): the
        step runs on the cached encodings -- no video projection, no video recurrence, none of the encoder's training saves.  The
        video encoder must be frozen (Trainer(freeze=('video_encoder',)) / requires_grad = False on its eight tensors), else
        ValueError before anything is enqueued; its tensors report untouched and keep weights, moments, step counts and torch
        version, so the cache is still fresh after the step.
        library (a ClipLibrary, with video=None and video_index = the library row of every question's clip): the raw clip features
        stay on the device and one launch gathers the step's clips (VideoNMN.run_programs); the video encoder trains as on `video`,
        and the step is that step bit for bit.  question_ids (host int32 [sum(q_lens)]) with words (a data.WordTable) and
        question=None: the question rows are gathered from the table.  Either way the step's host-to-device traffic is row numbers.
        At world > 1 every rank holds the whole library and table; the exchange is unchanged.
        Returns (per-question decoder CE of the local shard, BatchResult)."""
        from . import losses as L
        n = len(programs)
        # the checks of the clips, once per step; what they refuse is refused here: nothing of the step has been enqueued or counted yet
        src = self.model._clip_source(n, video, video_index, video_len, clips, train=True, library=library)
        question = self.model._question_rows(question, question_ids, words, q_lens)
        if global_batch is None:
            global_batch = self.global_batch
        if global_batch is None and self.world > 1:           # ragged shards: the window is the SUM of the shard sizes
            import torch.distributed as dist
            cnt = torch.tensor([n], dtype=torch.int64, device=self.flat_g.device if dist.get_backend() == 'nccl' else 'cpu')
            dist.all_reduce(cnt, op=dist.ReduceOp.SUM)
            global_batch = int(cnt.item())
        G = global_batch or n
        self.check(wait=False)                                # a failed earlier step surfaces here at the latest
        self.flat_g.zero_()                                   # optimizer.zero_grad()
        gstep = [self.questions_seen + 1 + self.rank + i * self.world for i in range(n)]
        self.questions_seen += G
        if gstep[0] <= self.after_iters:                      # some questions still without decoder loss
            answers = torch.where(torch.tensor([g > self.after_iters for g in gstep], device=answers.device), answers,
                                  torch.full_like(answers, -1))
        if questions is not None and gstep[-1] >= self.before_iters:
            if isinstance(questions, L.GoldBatch):
                questions = questions.select([g < self.before_iters for g in gstep])
            else:
                questions = [q if g < self.before_iters else dict(q, sg_res_by_step={}) for q, g in zip(questions, gstep)]
        drop = (self.dropout, self.dropout_seed + self.iters * self.world + self.rank) if self.dropout > 0 else None
        supervised = questions is not None and self.module_loss_weight != 0
        prep = {}

        def prepare(res_):        # host side of the intermediate losses: needs the plan only, runs before the pass is enqueued
            prep['p'] = L.prepare_module_losses(self.model, res_, questions, no_intermediate=self.no_intermediate,
                                                window=self.contrastive_window, world=self.world, rank=self.rank,
                                                class_table=self.class_table, global_batch=G)
        res = self.model._run(src, programs, spans, question, q_lens, True, drop, prepare if supervised else None, True)
        extra = set()
        trainable = list(self.model._trainable)               # requires_grad of this step (the pass has synced it into the context)
        tl = res.touched()                                    # known from the plan: uploaded BEFORE the backward pass is enqueued
                                                              # (0 for a frozen weight, whatever the programs use)
        if supervised:
            res.zero_grad_arenas()
            self.module_losses, extra = L.launch_module_losses(self.model, res, prep['p'], self.module_loss_weight / G)
            if extra:
                tl = [t_ or (nme in extra) for t_, nme in zip(tl, self.model._weight_names)]
        t = self._mask_ring.upload(tl, self.touched.device)
        frozen = not all(trainable)
        tmask = self._train_ring.upload(trainable, self.touched.device) if frozen else None
        overlap = self._side is not None
        loss = res.backward(answers, self.decoder_loss_weight / G, keep_arenas=supervised,
                            ready_event=self._ev_ready if overlap else None)
        if self.inject_failure:
            res.status_word().fill_(1)
        if self.inject_nonfinite:
            self.flat_g[:1].fill_(float('inf'))
        self.guard.copy_(res.status_word())
        late_ev = None
        if self.allreduce_late_events is not None and self.world > 1:
            late_ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            self.allreduce_late_events.append(late_ev)
        e0 = e1 = None
        if self.allreduce_events is not None and self.world > 1:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
        # the exchange: gradients summed, mask OR-ed, status OR-ed -- over RCCL / xGMI; in two pieces when overlapped
        reduce_gradients(self.flat_g, t, self.world, self.bucket, self.comm, status=self.guard,
                         split=self.split if overlap else None, side_stream=self._side,
                         # (the injected inf is written after the pass: the early piece then waits for the whole stream)
                         ready_event=None if self.inject_nonfinite else self._ev_ready, late_events=late_ev)
        if e0 is not None:
            e1.record()
            self.allreduce_events.append((e0, e1))
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        clip = self.max_grad_norm is not None
        if clip:
            # norms of the REDUCED bucket (identical on every rank), the clip coefficient, and bit 1 of the guard when the
            # norm is not finite -- before the bookkeeping below reads the guard
            check(lib.stair_grad_norm(C.c_void_p(self.flat_g.data_ptr()), self.n, C.c_void_p(self._seg_first_block.data_ptr()),
                                      C.c_void_p(self._seg_numel.data_ptr()), self.seg_grad_norm.numel(), C.c_float(self.max_grad_norm),
                                      C.c_void_p(self._norm_scratch.data_ptr()), C.c_void_p(self.seg_grad_norm.data_ptr()),
                                      C.c_void_p(self.grad_norm.data_ptr()), C.c_void_p(self.guard.data_ptr()), stream))
        # bookkeeping of a step the guard refuses stays that of the last good step (on the device: the host does not wait)
        ok = (self.guard == 0).to(torch.int32)
        if self.skip_untouched == 'ever':
            self.touched = torch.maximum(self.touched, t * ok)
        else:
            self.touched.copy_(t)
        # Adam's mask: under 'ever' a parameter that was touched once and is frozen NOW is skipped too (its moments must not decay
        # into the weight); nothing is frozen -> the mask is self.touched itself, as it always was
        mask = self.touched * tmask if frozen else self.touched
        self.steps += (mask * ok).to(torch.float32)
        lr = self.lr * self.lr_factor()
        adam_args = (C.c_void_p(self.flat_p.data_ptr()), C.c_void_p(self.flat_g.data_ptr()),
                     C.c_void_p(self.exp_avg.data_ptr()), C.c_void_p(self.exp_avg_sq.data_ptr()),
                     C.c_void_p(self.seg_of_block.data_ptr()), C.c_void_p(mask.data_ptr()),
                     C.c_void_p(self.steps.data_ptr()), C.c_float(lr), C.c_float(self.betas[0]),
                     C.c_float(self.betas[1]), C.c_float(self.eps), C.c_float(self.wd), self.n,
                     C.c_void_p(self.guard.data_ptr()))           # guard: no update when ANY rank's pass failed
        if clip:       # gradient times the coefficient inside the kernel: flat_g keeps the unclipped gradient
            check(lib.stair_adam_step_scaled(*adam_args, C.c_void_p(self.grad_norm.data_ptr() + 4), stream))
        else:
            check(lib.stair_adam_step(*adam_args, stream))
        # the kernel wrote the parameters through their storage: tell torch, as an in-place torch update would (version counters --
        # what autograd's saved tensors and a ClipCache's staleness check go by)
        # -- for the parameters the kernel may have written only: a frozen encoder keeps its version, and a ClipCache made before the
        # run is still fresh after it.  (At world > 1 another rank's shard may have touched what this one's did not.)
        self._ever = [a or b for a, b in zip(self._ever, tl)]
        hit = trainable if self.world > 1 else [a and b for a, b in zip(trainable, self._ever if self.skip_untouched == 'ever' else tl)]
        written = [p for p, w in zip(self._params, hit) if w]
        if written:
            torch.autograd.graph.increment_version(written)
        if len(self._status) < 16:
            host = torch.empty(1, dtype=torch.int32).pin_memory()
        else:                                                 # the oldest entry's buffer is reused: look at it first
            self._raise_if_failed(*self._status[0])
            host = self._status.pop(0)[1]
        host.copy_(self.guard, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        self._status.append((self.iters, host, ev))
        if clip:
            if len(self._norms) >= 16:                        # nobody collects them: the oldest step's figures make room
                _, old, old_ev = self._norms.pop(0)
                old_ev.synchronize()
                self._norm_free.append(old)
            nhost = self._norm_free.pop() if self._norm_free else torch.empty(2, dtype=torch.float32).pin_memory()
            nhost.copy_(self.grad_norm, non_blocking=True)
            nev = torch.cuda.Event()
            nev.record()
            self._norms.append((self.iters, nhost, nev))
        self.iters += 1                                       # scheduler.step()
        return loss, res

    def _raise_if_failed(self, step, host, ev):
        from ._lib import StairError
        ev.synchronize()
        if int(host[0]) == 2:                                 # bit 1 alone: stair_grad_norm found the reduced bucket's norm inf or NaN
            self._status = []
            raise StairError('non-finite gradient norm in optimizer step %d; weights, moments and step counts are those of the last '
                             'good step' % step)
        if int(host[0]) != 0:
            self._status = []
            raise StairError('optimizer step %d was skipped on every rank: a cooperative LSTM recurrence timed out on at least one of '
                             'them (its workgroups were not co-resident -- another queue on that GPU?); weights, Adam moments and '
                             'per-tensor step counts are those of the last good step.  STAIR_LSTM_COOP=0 selects the '
                             'one-workgroup kernels' % step)

    def check(self, wait=True):
        """Raises StairError if a step reported a failed pass (bit 0: a cooperative LSTM hand-off that timed out, the gradients of
        that step held NaN; bit 1, with max_grad_norm: the norm of the reduced gradients was inf or NaN).  A caller may catch
        the error and go on with the next window.  The word it reads is the step's status summed over all ranks -- the one Adam's guard read -- so at
        world > 1 every rank raises for the same step, whichever rank failed, and none of them has applied the update:
        parameters, moments and per-tensor step counts are those of the last good step.  The host-side counters (`iters`, the
        LambdaLR position, and `questions_seen`) have advanced past the refused window, as the data loader has.
        wait=False looks only at steps the GPU has finished."""
        keep = []
        for entry in self._status:
            if not wait and not entry[2].query():
                keep.append(entry)
                continue
            self._raise_if_failed(*entry)
        self._status = keep[-16:]

    # ---- stopping and resuming ------------------------------------------------------------------------------------------------
    def _hyper(self):
        """the constructor arguments that change the trajectory, as a training state holds them (train_state.HYPER)"""
        from .train_state import plain
        return {'lr': self.lr, 'betas': plain(self.betas), 'eps': self.eps, 'weight_decay': self.wd,
                'scheduler_start_factor': self.sched[0], 'scheduler_end_factor': self.sched[1], 'scheduler_total_iters': self.sched[2],
                'skip_untouched': self.skip_untouched, 'dropout': self.dropout, 'dropout_seed': self.dropout_seed,
                'train_module_before_iters': self.before_iters, 'train_decoder_after_iters': self.after_iters,
                'decoder_loss_weight': self.decoder_loss_weight, 'module_loss_weight': self.module_loss_weight,
                'contrastive_window': self.contrastive_window, 'no_intermediate': plain(self.no_intermediate),
                'max_grad_norm': self.max_grad_norm}

    def state_dict(self):
        """The training state (stair_amd.train_state): both Adam moments, the per-tensor step counts, the touched mask and its host
        view, the trainable flags, `iters`, `questions_seen`, `world` and the trajectory-changing constructor arguments -- per weight
        NAME, unpadded, on the CPU.  Together with model.state_dict() (the weights are NOT in here) it is all a run needs to go on
        bit for bit; see load_state_dict for the order.

        SYNCHRONISES: it first calls check(wait=True), so a refused step raises StairError BEFORE a checkpoint is written (a second
        call then succeeds and holds the last good step, which is what the device holds by construction; `iters` and
        `questions_seen` have moved past the refused window, as check() documents), then copies the buffers to the host."""
        self.check(wait=True)
        names = self.model._weight_names
        m, v = self.exp_avg.cpu(), self.exp_avg_sq.cpu()
        steps, touched = self.steps.cpu().tolist(), self.touched.cpu().tolist()
        tensors = {}
        for i, (nme, p) in enumerate(zip(names, self._params)):
            lo, hi = self.offsets[i], self.offsets[i] + p.numel()
            if steps[i] != int(steps[i]):
                raise RuntimeError('step count of %s is %r, not a whole number' % (nme, steps[i]))
            tensors[nme] = {'exp_avg': m[lo:hi].clone().view(p.shape), 'exp_avg_sq': v[lo:hi].clone().view(p.shape),
                            'steps': int(steps[i]), 'touched': int(touched[i]), 'ever': bool(self._ever[i]),
                            'trainable': bool(p.requires_grad)}
        from .train_state import FORMAT
        return {'format': FORMAT, 'names': list(names), 'numels': [p.numel() for p in self._params], 'tensors': tensors,
                'iters': int(self.iters), 'questions_seen': int(self.questions_seen), 'world': int(self.world), 'hyper': self._hyper()}

    def load_state_dict(self, state, strict=True):
        """Puts a training state back (state_dict() of an earlier Trainer, data.load_trainer_state of a checkpoint, or
        train_state.from_torch_adam of a torch optimizer): exp_avg, exp_avg_sq, steps, touched, the host view of the mask, `iters`
        and `questions_seen`.  The order that works:

            model, config = data.load_checkpoint(ckpt_dir)      # the weights first ...
            model = model.to(device)
            trainer = Trainer(model, ...)                       # ... because the Trainer turns the parameters into views of its
            trainer.load_state_dict(data.load_trainer_state(ckpt_dir))      # flat buffer; then the state

        The state is validated as a whole first (train_state.validate) and NOTHING is written on any failure.  Weights,
        requires_grad flags and gradient buffers are never touched; a schedule that froze or thawed parameters re-applies its flags
        before this call.  Pending status words are checked (a refused step of THIS Trainer still raises StairError) and then
        dropped with the pending gradient-norm figures: they belong to the run that is being replaced.  Synchronises.

        strict=True (default): a trajectory-changing constructor argument (lr, betas, eps, weight_decay, the three scheduler numbers,
        skip_untouched, dropout, dropout_seed, train_module_before_iters, train_decoder_after_iters, decoder_loss_weight,
        module_loss_weight, contrastive_window, no_intermediate, max_grad_norm), `world`, or a trainable flag that differs
        between the state and this Trainer / model raises ONE ValueError listing every difference as `name: saved -> now`.
        strict=False: exactly those fields keep THIS Trainer's values -- a deliberate change of schedule --, moments, step counts,
        masks and counters are loaded all the same.
        At world > 1 every rank loads the same state."""
        from . import train_state as TS
        names = self.model._weight_names
        TS.validate(state, names, [p.numel() for p in self._params], {nme: tuple(p.shape) for nme, p in zip(names, self._params)})
        if strict:
            now, diffs = self._hyper(), []
            for key in TS.HYPER:
                if TS.plain(state['hyper'][key]) != now[key]:
                    diffs.append('%s: %r -> %r' % (key, state['hyper'][key], now[key]))
            if state['world'] != self.world:
                diffs.append('world: %r -> %r' % (state['world'], self.world))
            for nme, p in zip(names, self._params):
                if state['tensors'][nme]['trainable'] != bool(p.requires_grad):
                    diffs.append('%s.trainable: %r -> %r' % (nme, state['tensors'][nme]['trainable'], bool(p.requires_grad)))
            if diffs:
                raise ValueError('the training state was saved by another schedule (saved -> now): ' + '; '.join(diffs) +
                                 '.  Build the Trainer / set requires_grad as saved, or pass strict=False to keep the present values')
        self.check(wait=True)
        m, v = torch.zeros(self.n), torch.zeros(self.n)       # the padding between segments stays zero
        for i, (nme, p) in enumerate(zip(names, self._params)):
            t = state['tensors'][nme]
            m[self.offsets[i]: self.offsets[i] + p.numel()] = t['exp_avg'].reshape(-1)
            v[self.offsets[i]: self.offsets[i] + p.numel()] = t['exp_avg_sq'].reshape(-1)
        self.exp_avg.copy_(m)
        self.exp_avg_sq.copy_(v)
        self.steps.copy_(torch.tensor([float(state['tensors'][nme]['steps']) for nme in names]))
        self.touched.copy_(torch.tensor([state['tensors'][nme]['touched'] for nme in names], dtype=torch.int32))
        self._ever = [bool(state['tensors'][nme]['ever']) for nme in names]
        self.iters, self.questions_seen = int(state['iters']), int(state['questions_seen'])
        torch.cuda.synchronize(self.flat_p.device)
        self._status = []
        if self.seg_grad_norm is not None:
            self._norm_free += [host for _, host, _ in self._norms]
            self._norms = []

    def grad_norms_by_name(self):
        """{weight name: L2 norm of its reduced, unclipped gradient in the last step} -- 0.0 for tensors no program of the
        window touched.  Needs max_grad_norm; synchronises (a device -> host copy)."""
        if self.seg_grad_norm is None:
            raise RuntimeError('gradient norms are measured only with max_grad_norm (float("inf") measures without clipping)')
        return dict(zip(self.model._weight_names, self.seg_grad_norm.cpu().tolist()))

    def finished_grad_norms(self):
        """[(step, global gradient norm, clip coefficient)] of the steps the GPU has finished since the last call, oldest first;
        never waits.  The figures travel through a ring of page-locked buffers beside the status words: a caller that does
        not collect them loses all but the latest 16."""
        if self.seg_grad_norm is None:
            raise RuntimeError('gradient norms are measured only with max_grad_norm (float("inf") measures without clipping)')
        out = []
        while self._norms and self._norms[0][2].query():
            step, host, _ = self._norms.pop(0)
            out.append((step, float(host[0]), float(host[1])))
            self._norm_free.append(host)
        return out
