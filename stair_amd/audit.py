"""Audit pass: the supervised intermediate results of a finished batch decoded ON THE DEVICE into what a person reads, and scored
against gold where there is gold (csrc/audit.hip; include/stair_hip.h "Audit decoders").

    Localize / Temporal / ExistsFrame   -> the frame interval [start, end) around the attention peak; temporal IoU with the gold span
    Exists / Xor / Equals               -> the pretrain head's yes / no with its score; right or wrong
    Filter / ToAction / Superlative     -> the `top` nearest classes of a ClassTable; the rank of the best gold class

The audited nodes are those of ``losses.supervised_nodes(q, model.pretrain_modules)``; gold comes from ``q['sg_res_by_step']``
where present and not None -- a node without gold (a whole test split) is decoded all the same and not scored.

Host cost of ``audit_batch``: one pass over the questions (a per-question pack cached on the dict, gold through
``losses.compile_gold``), one gather through ``BatchResult.node_table()``, ONE staged upload, then one launch per decoder --
attention, each head module present (a head launch takes one weight), rank -- plus the class-table encoding; no per-node library
call and no synchronisation.  The outputs sit in one device buffer and come to the host in ONE copy when an array is first read.

Out of scope: FilterFrame (per-frame object sets; it keeps its loss only), sharding over ranks, hipGraph capture of the audit
launches, seconds instead of frames."""
from __future__ import annotations

import numpy as np
import torch

from . import losses as L
from . import ops

ATTENTION = ('Localize', 'Temporal', 'ExistsFrame')          # att_module codes 0, 1, 2 (losses.ATTENTION_KINDS)
HEADS = ('Exists', 'Xor', 'Equals')                          # head_module codes 0, 1, 2
CONTRASTIVE = ('Filter', 'ToAction', 'Superlative')          # cont_module codes 0, 1, 2
AUDITED = frozenset(ATTENTION + HEADS + CONTRASTIVE)
RECALL_AT = (0.3, 0.5, 0.7)


class _Pack:
    """The audited nodes of ONE question as arrays (token positions relative to its program, ascending), with their gold."""
    __slots__ = ('att', 'head', 'cont')

    def __init__(self, question, modules):
        prog = question['nmn_program_list']
        nodes = sorted((i, step) for step, i in L.supervised_nodes(question, modules).items() if prog[i] in AUDITED)
        att_gold, head_gold, cont_gold = {}, {}, {}
        if question.get('sg_res_by_step'):
            gp = L.compile_gold(question, modules & AUDITED)          # (the per-question cache of the criteria)
            att_gold = {int(p): iv for p, iv in zip(gp.att_pos, gp.att_iv)}
            for pos, lab in gp.head.values():
                head_gold.update(zip(pos.tolist(), lab.tolist()))
            cont_gold = {pos: [name for name, _ in gold] for pos, _, gold in gp.cont}
        none_iv = np.full((2, 2), np.nan)
        att = [(i, step, ATTENTION.index(prog[i]), i in att_gold, att_gold.get(i, none_iv)) for i, step in nodes if prog[i] in ATTENTION]
        head = [(i, step, HEADS.index(prog[i]), head_gold.get(i, -1)) for i, step in nodes if prog[i] in HEADS]
        cont = [(i, step, CONTRASTIVE.index(prog[i]), cont_gold.get(i)) for i, step in nodes if prog[i] in CONTRASTIVE]
        ints = lambda rows, w: np.asarray([r[:w] for r in rows], dtype=np.int64).reshape(-1, w)
        # one integer matrix per family (a batch is then one concatenation per family): position, program_idx, module code, gold flag / label
        self.att = (ints(att, 4), np.asarray([r[4] for r in att], dtype=np.float64).reshape(-1, 2, 2))
        self.head = ints(head, 4)
        self.cont = (ints(cont, 3), [r[3] for r in cont])


def _pack(question, modules):
    """_Pack of a question, cached on the dict (key '_audit_pack') as long as its sg_res_by_step object is the same."""
    key = (id(question.get('sg_res_by_step')), modules)
    hit = question.get('_audit_pack')
    if hit is not None and hit[0] == key:
        return hit[1]
    pack = _Pack(question, modules)
    question['_audit_pack'] = (key, pack)
    return pack


_FIELDS = ('start', 'end', 'peak', 'on', 'peak_value', 'iou', 'pred', 'score', 'correct', 'top', 'top_sim', 'rank', 'best_gold_sim')


class AuditBatch:
    """The decoded nodes of one batch as flat numpy arrays per family (module codes index ATTENTION / HEADS / CONTRASTIVE):
      attention, one entry per ROW (Localize with two keywords has two): att_q, att_pos, att_idx (program_idx), att_module,
        att_row (row of its node), att_gold [rows, 2] (NaN without gold) | start, end, peak, on, peak_value, iou (-1 without gold)
      heads, module by module (Exists, Xor, Equals), question order inside: head_q, head_pos, head_idx, head_module,
        label (-1 without gold) | pred, score, correct (-1 without gold)
      contrastive: cont_q, cont_pos, cont_idx, cont_module, gold_off [n + 1] / gold_cls (the gold classes of node i are
        gold_cls[gold_off[i]: gold_off[i + 1]]; cont_has_gold: a gold list was there, even an empty one) |
        top [n, k], top_sim [n, k], rank (0 without gold), best_gold_sim
    The arrays after `|` are computed on the device and fetched with ONE copy when the first of them is read (that read
    synchronises).  skipped: {module: nodes left out} -- the contrastive nodes of a call without class_table."""

    def __init__(self, host, device_buffer, views, skipped, top):
        self.__dict__.update(host)
        self._buf, self._views, self._fetched = device_buffer, views, None
        self.skipped, self.k = skipped, top

    def __getattr__(self, name):
        if name in _FIELDS:
            return self._fetch()[name]
        raise AttributeError(name)

    def _fetch(self):
        if self._fetched is None:
            raw = self._buf.cpu().numpy() if self._buf is not None else np.zeros(0, dtype=np.uint8)
            self._fetched = {name: raw[off: off + nbytes].view(dt).reshape(shape) for name, (off, nbytes, dt, shape) in self._views.items()}
            self._buf = None
        return self._fetched

    def records(self, questions, class_table=None, ids=None):
        """{qa_id: {program_idx: {...}}}, the key layout of evaluate.filter_text_results (qa_id: q['qa_id'], else ids[i], else i):
          attention  {'module', 'interval': [(start, end)], 'peak': [..], 'on': [..], 'peak_value': [..], 'iou': [..] | None,
                      'gold': [(start, end)] | None}        one list entry per row, frames
          head       {'module', 'pred': bool, 'score', 'gold': bool | None, 'correct': bool | None}
          contrastive {'module', 'top': [class names], 'top_sim': [..], 'rank': int | None, 'best_gold_sim': float | None,
                      'gold': [class names] | None}        (class ids instead of names without class_table)"""
        key = lambda qi: questions[qi].get('qa_id', ids[qi] if ids is not None else qi)
        out = {key(qi): {} for qi in range(len(questions))}
        name = (lambda c: class_table.names[c] if 0 <= c < len(class_table) else None) if class_table is not None else int
        f = self._fetch()
        for r in range(self.att_q.size):
            node = out[key(int(self.att_q[r]))].setdefault(int(self.att_idx[r]), {
                'module': ATTENTION[self.att_module[r]], 'interval': [], 'peak': [], 'on': [], 'peak_value': [], 'iou': [], 'gold': []})
            gold = f['iou'][r] >= 0
            node['interval'].append((int(f['start'][r]), int(f['end'][r])))
            node['peak'].append(int(f['peak'][r])); node['on'].append(int(f['on'][r]))
            node['peak_value'].append(float(f['peak_value'][r]))
            node['iou'].append(float(f['iou'][r]) if gold else None)
            node['gold'].append((float(self.att_gold[r, 0]), float(self.att_gold[r, 1])) if gold else None)
        for per_q in out.values():
            for node in per_q.values():
                if 'interval' in node and node['gold'][0] is None:
                    node['iou'] = node['gold'] = None
        for i in range(self.head_q.size):
            gold = self.label[i] >= 0
            out[key(int(self.head_q[i]))][int(self.head_idx[i])] = {
                'module': HEADS[self.head_module[i]], 'pred': bool(f['pred'][i]), 'score': float(f['score'][i]),
                'gold': bool(self.label[i]) if gold else None, 'correct': bool(f['correct'][i]) if gold else None}
        for i in range(self.cont_q.size):
            scored = f['rank'][i] > 0
            out[key(int(self.cont_q[i]))][int(self.cont_idx[i])] = {
                'module': CONTRASTIVE[self.cont_module[i]], 'top': [name(int(c)) for c in f['top'][i]],
                'top_sim': [float(v) for v in f['top_sim'][i]], 'rank': int(f['rank'][i]) if scored else None,
                'best_gold_sim': float(f['best_gold_sim'][i]) if scored else None,
                'gold': [name(int(c)) for c in self.gold_cls[self.gold_off[i]: self.gold_off[i + 1]]] if self.cont_has_gold[i] else None}
        return out


def audit_batch(model, res, questions, class_table=None, threshold=0.5, top=5):
    """Decode and score the supervised nodes of a finished pass.  res: the BatchResult of a forward_batch of these questions (an
    inference plan; a training plan is read the same way and not modified).  class_table (losses.ClassTable): what the
    contrastive nodes are ranked against -- without it they are left out (AuditBatch.skipped).  threshold: a frame of an
    attention row is on from this value; top: classes kept per contrastive node.  Returns an AuditBatch."""
    if len(questions) != res.info.n_questions:
        raise ValueError('%d questions for a plan of %d' % (len(questions), res.info.n_questions))
    if top < 1:
        raise ValueError('top must be at least 1')
    dev = res.pred.device
    H, T = model.config['hidden_size'], res.info.T
    modules = frozenset(model.pretrain_modules)
    packs = [_pack(q, modules) for q in questions]
    _, slot_t, aux_t, _, rel_t = res.node_table()
    base = np.asarray(res._prog_off, dtype=np.int64)
    i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)

    def cat(parts, width):
        """(rows of the questions' matrices, the question of every row)"""
        sizes = np.fromiter((p.shape[0] for p in parts), dtype=np.int64, count=len(parts))
        full = [p for p in parts if p.shape[0]]
        return (np.concatenate(full) if full else np.zeros((0,) + width, dtype=parts[0].dtype if parts else np.int64)), np.repeat(np.arange(len(parts)), sizes)
    host, up, where = {}, [], {}

    def stage(key, *arrays):
        where[key] = (len(up), len(arrays))
        up.extend(arrays)

    # ---- attention rows (Localize: K = aux rows at its slot; Temporal: its related_attn row; ExistsFrame: its row) ----
    a_int, a_q = cat([p.att[0] for p in packs], (4,))
    a_pos, a_idx, a_mod, a_has = a_int[:, 0], a_int[:, 1], a_int[:, 2], a_int[:, 3].astype(np.int32)
    a_iv = cat([p.att[1] for p in packs], (2, 2))[0]
    n_att = int(a_pos.size)
    tok = a_pos + base[a_q]
    a_slot = np.where(a_mod == 1, rel_t[tok], slot_t[tok])
    a_K = np.where(a_mod == 0, aux_t[tok], 1).astype(np.int64)
    item = np.repeat(np.arange(n_att), a_K)
    row = np.arange(item.size) - np.repeat(np.concatenate([[0], np.cumsum(a_K)])[:-1], a_K)
    qf = res.question_frames
    a_len = i32(np.asarray(qf)[a_q]) if qf is not None else None
    row_iv = a_iv[item, row] if n_att else np.zeros((0, 2))                  # a node whose gold holds fewer intervals than rows: (0, 0), as the criterion
    row_gold = a_has[item].astype(bool)
    if row_gold.any():
        g = np.flatnonzero(row_gold)
        L.refuse_unindexable_ends(row_iv[g, 1], (a_len[item[g]] if qf is not None else np.full(g.size, T)), lambda j: (
            '%s at program position %d of question %d' % (ATTENTION[a_mod[item[g[j]]]], a_pos[item[g[j]]], a_q[item[g[j]]])))
    host.update(att_q=a_q[item], att_pos=a_pos[item], att_idx=a_idx[item], att_module=a_mod[item], att_row=row,
                att_gold=np.where(row_gold[:, None], row_iv, np.nan))
    if n_att:
        stage('att', i32(a_slot), i32(a_K), i32(np.concatenate([[0], np.cumsum(a_K)])), np.ascontiguousarray(np.where(row_gold[:, None], row_iv, 0.0)),
              i32(a_has), *([a_len] if a_len is not None else []))
    # ---- heads, module by module ----
    h_int, h_q = cat([p.head for p in packs], (4,))
    order = np.argsort(h_int[:, 2], kind='stable')
    h_int, h_q = h_int[order], h_q[order]
    h_pos, h_idx, h_mod, h_lab = h_int[:, 0], h_int[:, 1], h_int[:, 2], h_int[:, 3].astype(np.int32)
    n_head = int(h_pos.size)
    if n_head and not model.config['have_pretrain_head']:
        raise RuntimeError('%s loss needs have_pretrain_head (modules.py)' % HEADS[h_mod[0]])
    host.update(head_q=h_q, head_pos=h_pos, head_idx=h_idx, head_module=h_mod, label=h_lab)
    if n_head:
        stage('head', i32(slot_t[h_pos + base[h_q]]), i32(h_lab))
    # ---- contrastive nodes against the class table ----
    c_int, c_q = cat([p.cont[0] for p in packs], (3,))
    c_pos, c_idx, c_mod = c_int[:, 0], c_int[:, 1], c_int[:, 2]
    c_gold = [g for p in packs for g in p.cont[1]]
    skipped = {}
    if class_table is None:
        for m in c_mod:
            skipped[CONTRASTIVE[m]] = skipped.get(CONTRASTIVE[m], 0) + 1
        c_q, c_pos, c_idx, c_mod, c_gold = c_q[:0], c_pos[:0], c_idx[:0], c_mod[:0], []
    n_cont = int(c_pos.size)
    try:
        g_cls = i32([class_table.index[n] for g in c_gold if g for n in g])
    except KeyError as e:
        raise KeyError('class %s is not in the ClassTable (build it from the whole dataset: ClassTable.from_questions)' % e)
    g_off = i32(np.concatenate([[0], np.cumsum([len(g) if g else 0 for g in c_gold])]))
    host.update(cont_q=c_q, cont_pos=c_pos, cont_idx=c_idx, cont_module=c_mod, gold_off=g_off, gold_cls=g_cls,
                cont_has_gold=np.asarray([g is not None for g in c_gold], dtype=bool))
    k = min(int(top), len(class_table)) if n_cont else 0
    if n_cont:
        stage('cont', i32(slot_t[c_pos + base[c_q]]), g_off, *([g_cls] if g_cls.size else []))
    # ---- ONE upload, one output buffer ----
    staging = model.__dict__.setdefault('_loss_staging', L._Staging())
    d = staging.upload(up, dev) if up else []
    got = lambda key: d[where[key][0]: where[key][0] + where[key][1]]
    n_rows = int(item.size)
    layout = [('start', np.int32, (n_rows,)), ('end', np.int32, (n_rows,)), ('peak', np.int32, (n_rows,)), ('on', np.int32, (n_rows,)),
              ('peak_value', np.float32, (n_rows,)), ('iou', np.float32, (n_rows,)),
              ('pred', np.int32, (n_head,)), ('score', np.float32, (n_head,)), ('correct', np.int32, (n_head,)),
              ('top', np.int32, (n_cont, k)), ('top_sim', np.float32, (n_cont, k)), ('rank', np.int32, (n_cont,)),
              ('best_gold_sim', np.float32, (n_cont,))]
    views, total = {}, 0
    for name, dt, shape in layout:
        nbytes = int(np.prod(shape)) * 4
        views[name] = (total, nbytes, dt, shape)
        total += (nbytes + 15) // 16 * 16
    buf = torch.empty(total, dtype=torch.uint8, device=dev) if total else None
    tdt = {np.int32: torch.int32, np.float32: torch.float32}
    out = lambda *names: [buf[views[n][0]: views[n][0] + views[n][1]].view(tdt[views[n][2]]).view(views[n][3]) for n in names]
    # ---- the launches ----
    if n_att:
        slot_d, K_d, off_d, iv_d, has_d = got('att')[:5]
        len_d = got('att')[5] if a_len is not None else None
        ops.audit_attention(res._arena(res.info.att_off, res.info.n_att, T), slot_d, K_d, off_d, n_rows, threshold, lens=len_d,
                            intervals=iv_d if row_gold.any() else None, has_gold=has_d,
                            out=out('start', 'end', 'peak', 'on', 'peak_value', 'iou'))
    vec = res._arena(res.info.vec_off, res.info.n_vec, H)
    if n_head:
        slot_d, lab_d = got('head')
        pred_d, score_d, correct_d = out('pred', 'score', 'correct')
        for code, module in enumerate(HEADS):
            lo, hi = np.searchsorted(h_mod, [code, code + 1])
            if hi > lo:
                head = model.submodules[module].pretrain_head
                ops.audit_head(vec, slot_d[lo:hi], head.weight.detach(), head.bias.detach(), label=lab_d[lo:hi],
                               out=(pred_d[lo:hi], score_d[lo:hi], correct_d[lo:hi]))
    if n_cont:
        # class representations: text encoder + L2Normalize, encoded once per call as prepare_module_losses encodes its table
        x, seq_off, max_len = class_table.device_rows(dev, model.config['text_size'])
        with torch.no_grad():
            _, h_n = ops.lstm_bidir(x, seq_off, max_len, [w.detach() for w in model._lstm_weights('text_encoder')])
            reps = ops.l2normalize(h_n)
        c = got('cont')
        ops.audit_rank(vec, c[0], reps, k, gold_off=c[1], gold_cls=c[2] if g_cls.size else None, gold_cls_host=g_cls if g_cls.size else None,
                       out=out('top', 'top_sim', 'rank', 'best_gold_sim'))
    return AuditBatch(host, buf, views, skipped, k)


def module_report(kind, values, top=5):
    """The figures of one module from its per-node values, float64 on the host: kind 'attention' (values = iou per row, -1 unscored),
    'head' (values = correct per node, -1 unscored) or 'contrastive' (values = rank per node, 0 unscored).  A module without a
    scored node reports n_scored = 0 and NaN."""
    v = np.asarray(values, dtype=np.float64)
    nan = float('nan')
    mean = lambda a: float(a.mean()) if a.size else nan
    if kind == 'attention':
        s = v[v >= 0]
        rep = {'n': int(v.size), 'n_scored': int(s.size), 'mean_iou': mean(s)}
        rep.update({'recall@%.1f' % b: mean((s >= b).astype(np.float64)) for b in RECALL_AT})
        return rep
    if kind == 'head':
        s = v[v >= 0]
        return {'n': int(v.size), 'n_scored': int(s.size), 'accuracy': mean(s)}
    s = v[v > 0]
    return {'n': int(v.size), 'n_scored': int(s.size), 'hit@1': mean((s <= 1).astype(np.float64)), 'hit@top': mean((s <= top).astype(np.float64)),
            'mrr': mean(1.0 / s)}


def module_values(batch):
    """{module: (kind, per-node values)} of an AuditBatch: what module_report takes, for every module the batch holds a node of."""
    out = {}
    for kind, names, codes, values in (('attention', ATTENTION, batch.att_module, batch.iou), ('head', HEADS, batch.head_module, batch.correct),
                                       ('contrastive', CONTRASTIVE, batch.cont_module, batch.rank)):
        for code, module in enumerate(names):
            m = codes == code
            if m.any():
                out[module] = (kind, np.asarray(values)[m])
    return out
