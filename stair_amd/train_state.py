"""The training state of a `stair_amd.train.Trainer`: what has to be written out, besides the weights, for a run that is
stopped and picked up again to end with the bits of one that never stopped ("Stopping and resuming").

A state is a plain dict -- dict, list, str, int, float, bool, None and CPU tensors only, so that
`torch.load(..., weights_only=True)` reads it back and a state file cannot run code:

    format           1
    names, numels    the canonical weight names (VideoNMN._weight_names) and their element counts
    tensors          {name: {exp_avg, exp_avg_sq   fp32, UNPADDED, in the parameter's own shape
                             steps                 int: Adam steps this tensor has taken
                             touched               int: the device mask Adam reads ('ever': has had a gradient)
                             ever                  bool: the host's view of the same
                             trainable             bool: requires_grad when the state was taken}}
    iters            optimizer steps taken: the LambdaLR position and, with dropout_seed, world and rank, the dropout masks
    questions_seen   what gates the two loss families (train_module_before_iters / train_decoder_after_iters)
    world            number of ranks
    hyper            every constructor argument of the Trainer that changes the trajectory (HYPER)

Everything is kept BY NAME: the order of the Trainer's flat buffers and the 256-float padding of their segments are its own
business, and a state written today loads into a Trainer that lays them out differently.

Nothing here needs a GPU: the functions are pure functions over such dicts, plus an atomic `save` and a refusing `load`.
`to_torch_adam` / `from_torch_adam` translate to and from the `state_dict()` of `torch.optim.Adam`, so that a run can move
to or from a loop written with torch's own optimizer.
"""
from __future__ import annotations

import math
import os
import pickle

import torch

FORMAT = 1
STATE_FILE = 'trainer_state.bin'

# constructor arguments of Trainer that change the trajectory, with the Trainer's defaults (dropout: None = the model's own)
HYPER = {'lr': 2e-4, 'betas': [0.9, 0.999], 'eps': 1e-8, 'weight_decay': 0.0,
         'scheduler_start_factor': 1.0, 'scheduler_end_factor': 0.1, 'scheduler_total_iters': 200000,
         'skip_untouched': 'ever', 'dropout': 0.0, 'dropout_seed': 0,
         'train_module_before_iters': 1e10, 'train_decoder_after_iters': 0,
         'decoder_loss_weight': 1.0, 'module_loss_weight': 1.0, 'contrastive_window': 32, 'no_intermediate': ['FilterFrame'],
         'max_grad_norm': None}
_TENSOR_FIELDS = ('exp_avg', 'exp_avg_sq', 'steps', 'touched', 'ever', 'trainable')


def plain(v):
    """tuples -> lists, all the way down: the form a value has in a state (and after a round trip through a file)"""
    if isinstance(v, (tuple, list)):
        return [plain(x) for x in v]
    return v


def _is_int(v):
    return isinstance(v, int) and not isinstance(v, bool)


def validate(state, names, numels, shapes=None):
    """Checks a state against the weight table it is meant for -- names and numels in weight-table order, optionally
    shapes {name: shape} -- BEFORE anything of it is written anywhere.  Every failure is a ValueError that names the weight
    and the field.  Checked: the format number; the name set and the element counts; per weight the presence and type of
    every field, moments fp32 with the right element count (and shape), the two moments of one shape, finite, exp_avg_sq >= 0,
    steps >= 0; under skip_untouched = 'ever' (the SAVED mode: under 'window' the mask is per step and says nothing about the
    past) a weight with touched == 0 has steps == 0 and zero moments; the counters; the hyper-parameters' names."""
    if not isinstance(state, dict):
        raise ValueError('a training state is a dict, got %s' % type(state).__name__)
    if state.get('format') != FORMAT:
        raise ValueError('training state: format is %r, this version reads format %d' % (state.get('format'), FORMAT))
    for key in ('names', 'numels', 'tensors', 'iters', 'questions_seen', 'world', 'hyper'):
        if key not in state:
            raise ValueError('training state: field %r is missing' % key)
    names, numels = list(names), [int(n) for n in numels]
    want, have = set(names), set(state['tensors'] if isinstance(state['tensors'], dict) else ())
    if not isinstance(state['tensors'], dict) or set(state['names']) != have or len(state['names']) != len(have) \
            or len(state['numels']) != len(state['names']):
        raise ValueError("training state: 'names', 'numels' and the keys of 'tensors' disagree")
    missing, extra = [n for n in names if n not in have], [n for n in state['names'] if n not in want]
    if missing or extra:
        raise ValueError('training state: the weight names do not fit this model: missing %s, unexpected %s'
                         % (missing or 'none', extra or 'none'))
    saved_numel = dict(zip(state['names'], state['numels']))
    hyper = state['hyper']
    if not isinstance(hyper, dict) or set(hyper) != set(HYPER):
        got = set(hyper) if isinstance(hyper, dict) else set()
        raise ValueError("training state: 'hyper' must hold exactly %s; missing %s, unexpected %s"
                         % (sorted(HYPER), sorted(set(HYPER) - got) or 'none', sorted(got - set(HYPER)) or 'none'))
    if hyper['skip_untouched'] not in ('ever', 'window'):
        raise ValueError("training state: hyper.skip_untouched is %r, not 'ever' or 'window'" % (hyper['skip_untouched'],))
    ever_mode = hyper['skip_untouched'] == 'ever'
    for key in ('iters', 'questions_seen'):
        if not _is_int(state[key]) or state[key] < 0:
            raise ValueError('training state: %s must be a non-negative int, got %r' % (key, state[key]))
    if not _is_int(state['world']) or state['world'] < 1:
        raise ValueError('training state: world must be a positive int, got %r' % (state['world'],))
    for name, numel in zip(names, numels):
        t = state['tensors'][name]
        if not isinstance(t, dict) or set(t) != set(_TENSOR_FIELDS):
            raise ValueError('training state: %s must hold exactly the fields %s' % (name, ', '.join(_TENSOR_FIELDS)))
        if saved_numel[name] != numel:
            raise ValueError('training state: %s: numels says %r elements, the model has %d' % (name, saved_numel[name], numel))
        for field in ('exp_avg', 'exp_avg_sq'):
            m = t[field]
            if not isinstance(m, torch.Tensor):
                raise ValueError('training state: %s.%s is not a tensor' % (name, field))
            if m.device.type != 'cpu':
                raise ValueError('training state: %s.%s lies on %s, not on the CPU' % (name, field, m.device))
            if m.dtype != torch.float32:
                raise ValueError('training state: %s.%s has dtype %s, not torch.float32' % (name, field, m.dtype))
            if m.numel() != numel or (shapes is not None and tuple(m.shape) != tuple(shapes[name])):
                raise ValueError('training state: %s.%s has shape %s, the model wants %s'
                                 % (name, field, tuple(m.shape), tuple(shapes[name]) if shapes is not None else '%d elements' % numel))
            if not bool(torch.isfinite(m).all()):
                raise ValueError('training state: %s.%s holds inf or NaN' % (name, field))
        if t['exp_avg'].shape != t['exp_avg_sq'].shape:
            raise ValueError('training state: %s.exp_avg_sq has shape %s, exp_avg has %s'
                             % (name, tuple(t['exp_avg_sq'].shape), tuple(t['exp_avg'].shape)))
        if numel and float(t['exp_avg_sq'].min()) < 0:
            raise ValueError('training state: %s.exp_avg_sq has a negative entry' % name)
        if not _is_int(t['steps']) or t['steps'] < 0:
            raise ValueError('training state: %s.steps must be a non-negative int, got %r' % (name, t['steps']))
        if t['touched'] not in (0, 1) or isinstance(t['touched'], bool):
            raise ValueError('training state: %s.touched must be 0 or 1, got %r' % (name, t['touched']))
        for field in ('ever', 'trainable'):
            if not isinstance(t[field], bool):
                raise ValueError('training state: %s.%s must be a bool, got %r' % (name, field, t[field]))
        if ever_mode and t['touched'] == 0:
            if t['steps'] != 0:
                raise ValueError("training state: %s.steps is %d although touched is 0 (skip_untouched = 'ever')" % (name, t['steps']))
            for field in ('exp_avg', 'exp_avg_sq'):
                if numel and float(t[field].abs().max()) != 0.0:
                    raise ValueError("training state: %s.%s is not zero although touched is 0 (skip_untouched = 'ever')" % (name, field))


# ---------------------------------------------------------------------------------------------------------------------
# files
# ---------------------------------------------------------------------------------------------------------------------
def atomic_write(path, write, mode='wb'):
    """`write(f)` into a temporary name beside `path`, flush, fsync, then os.replace: a job that is killed while it saves leaves
    the previous file whole (and at worst a stray `<name>.tmp.<pid>`)."""
    tmp = '%s.tmp.%d' % (path, os.getpid())
    try:
        with open(tmp, mode) as f:
            write(f)
            f.flush()
            os.fsync(f.fileno())
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
    try:                                        # the rename itself reaches the disk with the directory (where the platform allows)
        fd = os.open(os.path.dirname(os.path.abspath(path)), os.O_RDONLY)
        try:
            os.fsync(fd)
        finally:
            os.close(fd)
    except OSError:
        pass


def save(path, state):
    """Writes the state with torch.save, atomically (atomic_write)."""
    atomic_write(path, lambda f: torch.save(state, f))


def load(path):
    """The state of a file written by `save` -- tensors and plain containers only (torch.load(weights_only=True)): a file that
    names anything else is refused, not executed.  What the dict holds is checked by `validate`, against the model it is for."""
    try:
        state = torch.load(path, map_location='cpu', weights_only=True)
    except pickle.UnpicklingError as e:
        raise ValueError('%s is not a training state (a dict of tensors, numbers, strings and lists, as '
                         'stair_amd.train_state.save writes it); nothing of it was executed' % path) from e
    if not isinstance(state, dict) or 'format' not in state or not isinstance(state.get('tensors'), dict):
        raise ValueError('%s does not hold a training state' % path)
    return state


# ---------------------------------------------------------------------------------------------------------------------
# torch.optim.Adam
# ---------------------------------------------------------------------------------------------------------------------
_PROBE = None


def _adam_probe():
    """(param group, state entry) of a torch.optim.Adam of the installed torch after one step: which keys a group has and
    what a `step` looks like (an int up to torch 1.11, a scalar tensor since) are torch's to decide."""
    global _PROBE
    if _PROBE is None:
        p = torch.nn.Parameter(torch.zeros(1))
        opt = torch.optim.Adam([p])
        p.grad = torch.ones(1)
        opt.step()
        sd = opt.state_dict()
        _PROBE = (sd['param_groups'][0], sd['state'][0])
    return _PROBE


def to_torch_adam(state, param_names):
    """(state_dict for torch.optim.Adam.load_state_dict, iters).  param_names[i] names the optimizer's parameter i -- the order
    of model.parameters(), every tensor once.  Exact for skip_untouched = 'ever', which is torch 1.13's behaviour: Adam creates
    a parameter's state at its first gradient, so a tensor the mask has never seen gets NO entry and every other one
    `step`, `exp_avg`, `exp_avg_sq` (under 'window' the entry exists once the tensor has taken a step).  The group's `lr` is the
    BASE learning rate; the LambdaLR position is `iters`, returned beside the dict -- the caller's scheduler starts there.
    The remaining keys of the group are those of a default torch.optim.Adam of the installed torch."""
    group, entry = _adam_probe()
    hyper = state['hyper']
    ever_mode = hyper['skip_untouched'] == 'ever'
    out = {}
    for i, name in enumerate(param_names):
        if name not in state['tensors']:
            raise ValueError('to_torch_adam: the state has no weight named %s' % name)
        t = state['tensors'][name]
        if not (t['touched'] if ever_mode else t['steps'] > 0):
            continue
        step = entry['step']
        step = torch.tensor(float(t['steps']), dtype=step.dtype) if isinstance(step, torch.Tensor) else int(t['steps'])
        out[i] = {'step': step, 'exp_avg': t['exp_avg'].clone(), 'exp_avg_sq': t['exp_avg_sq'].clone()}
    group = dict(group, lr=hyper['lr'], betas=tuple(hyper['betas']), eps=hyper['eps'], weight_decay=hyper['weight_decay'],
                 params=list(range(len(param_names))))
    group.pop('initial_lr', None)
    return {'state': out, 'param_groups': [group]}, state['iters']


def from_torch_adam(optimizer_state_dict, param_names, shapes=None, iters=0, questions_seen=0, world=1, trainable=None, **hyper):
    """A training state from the state_dict() of a torch.optim.Adam with ONE parameter group (no amsgrad, no maximize).
    param_names[i] names the optimizer's parameter i.  lr (the base rate: pass iters for the scheduler's position), betas, eps and
    weight_decay come from the group; every other trajectory-changing argument of the Trainer from **hyper, with the Trainer's
    defaults (dropout: 0.0).  A parameter without an entry has never had a gradient: touched 0, zero moments -- in the shape
    `shapes[name]`, which only such parameters need.  trainable: {name: bool}, default all True."""
    groups = optimizer_state_dict['param_groups']
    if len(groups) != 1:
        raise ValueError('from_torch_adam: one parameter group expected, the optimizer has %d' % len(groups))
    group = groups[0]
    if group.get('amsgrad') or group.get('maximize'):
        raise ValueError('from_torch_adam: amsgrad and maximize have no counterpart in the Trainer')
    if list(group['params']) != list(range(len(param_names))):
        raise ValueError('from_torch_adam: the group lists %d parameters, param_names has %d' % (len(group['params']), len(param_names)))
    unknown = set(hyper) - set(HYPER)
    if unknown or set(hyper) & {'lr', 'betas', 'eps', 'weight_decay'}:
        raise ValueError('from_torch_adam: %s' % ('unknown arguments %s' % sorted(unknown) if unknown else
                                                  'lr, betas, eps and weight_decay are read from the optimizer'))
    h = dict(HYPER, **{k: plain(v) for k, v in hyper.items()})
    h.update(lr=float(group['lr']), betas=[float(b) for b in group['betas']], eps=float(group['eps']),
             weight_decay=float(group['weight_decay']))
    if h['max_grad_norm'] is not None:
        h['max_grad_norm'] = float(h['max_grad_norm'])
    tensors, numels = {}, []
    for i, name in enumerate(param_names):
        e = optimizer_state_dict['state'].get(i)
        if e is None:
            if shapes is None or name not in shapes:
                raise ValueError('from_torch_adam: %s has no optimizer state (no gradient so far): its shape must come in `shapes`' % name)
            zero = torch.zeros(tuple(shapes[name]), dtype=torch.float32)
            t = {'exp_avg': zero, 'exp_avg_sq': zero.clone(), 'steps': 0, 'touched': 0, 'ever': False}
        else:
            step = float(e['step'])
            if step != math.floor(step):
                raise ValueError('from_torch_adam: %s.step is %r, not a whole number' % (name, step))
            t = {'exp_avg': e['exp_avg'].detach().to('cpu', torch.float32).clone(),
                 'exp_avg_sq': e['exp_avg_sq'].detach().to('cpu', torch.float32).clone(), 'steps': int(step), 'touched': 1, 'ever': True}
        t['trainable'] = True if trainable is None else bool(trainable.get(name, True))
        tensors[name] = t
        numels.append(t['exp_avg'].numel())
    return {'format': FORMAT, 'names': list(param_names), 'numels': numels, 'tensors': tensors, 'iters': int(iters),
            'questions_seen': int(questions_seen), 'world': int(world), 'hyper': h}
