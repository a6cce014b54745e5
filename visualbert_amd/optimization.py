"""BertAdam and the LR schedules of the reference, with the update running as ONE fused multi-tensor
HIP kernel sequence over the flat parameter arena (visualbert_amd/csrc/optim.hip).

API mirrors visualbert/pytorch_pretrained_bert/optimization.py:
  _LRSchedule / ConstantLR / WarmupCosineSchedule / WarmupConstantSchedule / WarmupLinearSchedule (:37-173),
  BertAdam(params, lr, warmup, t_total, schedule, b1, b2, e, weight_decay, max_grad_norm) (:185-304).
Like the reference, BertAdam reads lr, schedule, b1, b2, e, weight_decay and max_grad_norm from EACH parameter group
(:262-301).  The hyper-parameters travel to the kernel as a device-resident table with one row per group
(include/visualbert_hip.h: vb_bert_adam_step_groups); a tensor's group id sits in its tensor-table entry.  The host image
of the table is rebuilt from `param_groups` at every step() and uploaded only when it differs from the last upload, so
`group["lr"] *= 0.5` between steps takes effect at the next step and an unchanged configuration costs no copy.
The kernel evaluates all six schedule classes of :83-173 in double from each tensor's OWN step counter (read before
its increment, :292,297).  Only a group whose schedule is a user subclass of _LRSchedule gets its multiplier from the
host (`schedule.get_lr(step)`, written into the group's row every step); that needs one common step count within the
group, which step() verifies.  When all groups share one set of hyper-parameters that the scalar entry vb_bert_adam_step can
express -- the reference's own training set-up: groups that differ in weight decay only, warmup-linear or constant -- step()
calls that entry instead: no table, and bit for bit the numbers this package has always given for that set-up (the scalar
entry carries warmup and t_total in fp32).  `layerwise_groups` builds the usual fine-tuning groups (layer-wise LR decay, head LR).

`Lamb` is the optimizer for large-batch training (You et al., "Large Batch Optimization for Deep Learning", with the NVLAMB
conventions): one global gradient-norm clip, optional bias correction, a trust ratio ||p|| / ||u|| per tensor.  It is BertAdam's
machinery -- arena, tables, group table, schedules, `touched` hand-over, state carry-over -- around another kernel entry
(include/visualbert_hip.h: vb_lamb_step_groups), whose group rows carry two more columns.
"""
import math
import re

import torch
from torch.optim import Optimizer

from . import _lib, ops


class _LRSchedule(object):
    warn_t_total = False

    def __init__(self, warmup=0.002, t_total=-1, **kw):
        if not 0.0 <= warmup < 1.0 and not warmup == -1:
            raise ValueError("Invalid warmup: {} - should be in [0.0, 1.0[ or -1".format(warmup))
        warmup = max(warmup, 0.)
        self.warmup, self.t_total = float(warmup), float(t_total)

    def get_lr(self, step, nowarn=False):
        if self.t_total < 0:
            return 1.
        return self.get_lr_(float(step) / self.t_total)

    def get_lr_(self, progress):
        return 1.


class ConstantLR(_LRSchedule):
    def get_lr_(self, progress):
        return 1.


class WarmupCosineSchedule(_LRSchedule):
    warn_t_total = True

    def __init__(self, warmup=0.002, t_total=-1, cycles=.5, **kw):
        super(WarmupCosineSchedule, self).__init__(warmup=warmup, t_total=t_total, **kw)
        self.cycles = cycles

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        progress = (progress - self.warmup) / (1 - self.warmup)
        return 0.5 * (1. + math.cos(math.pi * self.cycles * 2 * progress))


class WarmupCosineWithHardRestartsSchedule(WarmupCosineSchedule):
    """optimization.py:113-129: `cycles` cosine decays with hard restarts after the warm-up."""

    def __init__(self, warmup=0.002, t_total=-1, cycles=1., **kw):
        super(WarmupCosineWithHardRestartsSchedule, self).__init__(warmup=warmup, t_total=t_total, cycles=cycles, **kw)
        assert cycles >= 1.

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        progress = (progress - self.warmup) / (1 - self.warmup)
        return 0.5 * (1. + math.cos(math.pi * ((self.cycles * progress) % 1)))


class WarmupCosineWithWarmupRestartsSchedule(WarmupCosineWithHardRestartsSchedule):
    """optimization.py:132-150: training is cut into `cycles` equal parts, each with its own warm-up and cosine decay."""

    def __init__(self, warmup=0.002, t_total=-1, cycles=1., **kw):
        assert warmup * cycles < 1.
        warmup = warmup * cycles if warmup >= 0 else warmup
        super(WarmupCosineWithWarmupRestartsSchedule, self).__init__(warmup=warmup, t_total=t_total, cycles=cycles, **kw)

    def get_lr_(self, progress):
        progress = progress * self.cycles % 1.
        if progress < self.warmup:
            return progress / self.warmup
        progress = (progress - self.warmup) / (1 - self.warmup)
        return 0.5 * (1. + math.cos(math.pi * progress))


class WarmupConstantSchedule(_LRSchedule):
    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        return 1.


class WarmupLinearSchedule(_LRSchedule):
    warn_t_total = True

    def get_lr_(self, progress):
        if progress < self.warmup:
            return progress / self.warmup
        return max((progress - 1.) / (self.warmup - 1.), 0.)


SCHEDULES = {None: ConstantLR, "none": ConstantLR, "warmup_cosine": WarmupCosineSchedule,
             "warmup_constant": WarmupConstantSchedule, "warmup_linear": WarmupLinearSchedule}      # optimization.py:176-182
_SCHEDULE_CLASSES = {c.__name__: c for c in (ConstantLR, WarmupCosineSchedule, WarmupCosineWithHardRestartsSchedule,
                                             WarmupCosineWithWarmupRestartsSchedule, WarmupConstantSchedule,
                                             WarmupLinearSchedule)}


# schedule codes of the group table (include/visualbert_hip.h: vb_bert_adam_step_groups).  Exact classes only: a subclass may
# override get_lr_, so it is a user schedule and takes the host-multiplier code
_DEVICE_SCHEDULES = {ConstantLR: 0, WarmupLinearSchedule: 1, WarmupConstantSchedule: 2, WarmupCosineSchedule: 3,
                     WarmupCosineWithHardRestartsSchedule: 4, WarmupCosineWithWarmupRestartsSchedule: 5}
_HOST_SCHEDULE = 6
GROUP_COLS = 11         # lr, b1, b2, eps, weight_decay, max_grad_norm, schedule code, warmup, t_total, cycles, host multiplier
LAMB_GROUP_COLS = 13    # ... + bias_correction, always_adapt (include/visualbert_hip.h: vb_lamb_step_groups)


def _schedule_dict(sch):
    """what a checkpoint keeps of a schedule: the class name and its ATTRIBUTES (WarmupCosineWithWarmupRestartsSchedule holds
    warmup * cycles in `warmup`, optimization.py:139-141) -- a plain dict, torch.save-able by either side."""
    return {"class": type(sch).__name__, "warmup": float(getattr(sch, "warmup", -1)),
            "t_total": float(getattr(sch, "t_total", -1)), "cycles": getattr(sch, "cycles", None)}


def _schedule_from_dict(d):
    """the inverse of _schedule_dict: the saved values ARE the attributes, so they are set as attributes, not passed through
    the constructor again (which would multiply a restart schedule's warm-up by `cycles` a second time)."""
    cls = _SCHEDULE_CLASSES[d["class"]]
    sch = cls.__new__(cls)
    sch.warmup, sch.t_total = float(d["warmup"]), float(d["t_total"])
    if d.get("cycles") is not None:
        sch.cycles = d["cycles"]
    elif issubclass(cls, WarmupCosineSchedule):
        sch.cycles = 0.5 if cls is WarmupCosineSchedule else 1.
    return sch


def layerwise_groups(named_parameters, lr, layer_decay=1.0, head_lr=None, weight_decay=0.01):
    """Reference-style parameter groups for fine-tuning from a pre-trained encoder.  'pooler' parameters are dropped and
    the bias / LayerNorm names get weight_decay 0, exactly as ModelWrapper.initialize_opimizer does
    (models/model_wrapper.py:100-112).  Encoder layer i of L gets lr * layer_decay ** (L - 1 - i), the embeddings one factor
    more (layer_decay ** L), everything outside bert.embeddings / bert.encoder (the heads) gets `head_lr or lr`.
    Parameters with equal (lr, weight_decay) share a group, in the order of `named_parameters`: with layer_decay = 1 and no
    head_lr the result is the two groups of initialize_opimizer."""
    named = [(n, p) for n, p in named_parameters if "pooler" not in n]
    no_decay = ["bias", "LayerNorm.bias", "LayerNorm.weight"]
    layer_re = re.compile(r"(?:^|\.)bert\.encoder\.layer\.(\d+)\.")
    layer_of = {n: int(m.group(1)) for n, m in ((n, layer_re.search(n)) for n, _ in named) if m}
    n_layers = 1 + max(layer_of.values()) if layer_of else 0
    groups = {}
    for n, p in named:
        if n in layer_of:
            g_lr = lr * layer_decay ** (n_layers - 1 - layer_of[n])
        elif re.search(r"(?:^|\.)bert\.embeddings\.", n):
            g_lr = lr * layer_decay ** n_layers
        elif re.search(r"(?:^|\.)bert\.encoder\.", n):
            g_lr = lr                                   # encoder parameters above the layer stack
        else:
            g_lr = head_lr or lr
        wd = 0.0 if any(nd in n for nd in no_decay) else weight_decay
        groups.setdefault((g_lr, wd), {"params": [], "lr": g_lr, "weight_decay": wd})["params"].append(p)
    return list(groups.values())


class BertAdam(Optimizer):
    """BERT's Adam: per-tensor gradient clipping, no bias correction, decoupled weight decay, eps outside
    the sqrt, LR schedule evaluated from a per-tensor step counter (optimization.py:239-304).  Every parameter group
    carries its own lr, schedule, b1, b2, e, weight_decay and max_grad_norm.

    All parameters must live in one visualbert_amd ParameterArena (every model built by
    visualbert_amd.modeling does).  State (exp_avg = 'next_m', exp_avg_sq = 'next_v', step counters)
    is held as flat device buffers.

    `if p.grad is None: continue` (optimization.py:254-255) follows the zero_grad semantics of the reference's era
    (torch < 2: gradients are zeroed in place, so a parameter is skipped only until its first backward): a tensor that has
    ever received a gradient keeps stepping (weight decay, moment decay, counter) in steps that do not reach it.  Under
    torch >= 2's zero_grad(set_to_none=True) the reference itself would skip it again; `zero_grad()` here is one memset of
    the gradient arena either way.  load_state_dict keeps the moments / counters of parameters the checkpoint omits."""

    # what a subclass with another kernel entry (Lamb) changes: the width of a group row and the checkpoint names of the moments
    _group_cols = GROUP_COLS
    _moment_keys = ("next_m", "next_v")

    def _extra_defaults(self, kwargs):
        """per-group hyper-parameters beyond BertAdam's own."""
        return {}

    def _extra_columns(self, group):
        """the columns of a group's table row after the GROUP_COLS common ones."""
        return []

    def _ws_floats(self, nt, nc):
        return nt + nc

    def __init__(self, params, lr=None, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, **kwargs):
        if lr is None or lr < 0.0:
            raise ValueError("Invalid learning rate: {} - should be >= 0.0".format(lr))
        if not isinstance(schedule, _LRSchedule) and schedule not in SCHEDULES:
            raise ValueError("Invalid schedule parameter: {}".format(schedule))
        if not 0.0 <= b1 < 1.0:
            raise ValueError("Invalid b1 parameter: {} - should be in [0.0, 1.0[".format(b1))
        if not 0.0 <= b2 < 1.0:
            raise ValueError("Invalid b2 parameter: {} - should be in [0.0, 1.0[".format(b2))
        if not e >= 0.0:
            raise ValueError("Invalid epsilon value: {} - should be >= 0.0".format(e))
        if not isinstance(schedule, _LRSchedule):
            schedule = SCHEDULES[schedule](warmup=warmup, t_total=t_total)
        defaults = dict(lr=lr, schedule=schedule, b1=b1, b2=b2, e=e, weight_decay=weight_decay,
                        max_grad_norm=max_grad_norm)
        defaults.update(self._extra_defaults(kwargs))
        self._fused = None
        self.table_uploads = 0                           # host-to-device copies of the group table so far
        super(BertAdam, self).__init__(params, defaults)

    # -- fused state -------------------------------------------------------------------------------
    def _build(self):
        arena = None
        member = {}                                      # id(parameter) -> index of its group
        for gi, group in enumerate(self.param_groups):
            for p in group["params"]:
                a = getattr(p, "_vb_arena", None)
                if a is None:
                    raise RuntimeError("visualbert_amd.%s: parameter is not arena-managed (build the model with "
                                       "visualbert_amd.modeling; no per-tensor fallback exists)" % type(self).__name__)
                if arena is None:
                    arena = a
                elif a is not arena:
                    raise RuntimeError("visualbert_amd.%s: parameters from different arenas" % type(self).__name__)
                member[id(p)] = gi
        opt_flags = [id(p) in member for p in arena.params]
        dec_flags = [id(p) in member and self.param_groups[member[id(p)]]["weight_decay"] > 0.0 for p in arena.params]
        group_ids = [member.get(id(p), 0) for p in arena.params]
        tt, ct, nt, nc = arena.tables(opt_flags, dec_flags, group_ids)
        dev = arena.device
        self._fused = dict(arena=arena, tt=tt, ct=ct, nt=nt, nc=nc, n_groups=len(self.param_groups), group_ids=group_ids,
                           m=torch.zeros_like(arena.data), v=torch.zeros_like(arena.data),
                           norm2=torch.zeros(self._ws_floats(nt, nc), dtype=torch.float32, device=dev),
                           steps=torch.zeros(nt, dtype=torch.int32, device=dev),
                           # the group table: its device copy and the host image that copy was made from (None: not yet)
                           gt=torch.zeros(len(self.param_groups) * self._group_cols, dtype=torch.float64, device=dev),
                           gt_host=None,
                           opt_flags=opt_flags, dec_flags=dec_flags,
                           group_decays=[g["weight_decay"] > 0.0 for g in self.param_groups])
        return self._fused

    def _group_rows(self, f):
        """host image of the group table, from param_groups as they are NOW."""
        rows = []
        steps = None
        for gi, g in enumerate(self.param_groups):
            sch = g["schedule"]
            code = _DEVICE_SCHEDULES.get(type(sch), _HOST_SCHEDULE)
            mult = 1.0
            if code == _HOST_SCHEDULE:
                # a user schedule is a Python object: one multiplier per group and step, from ONE step count -- the counters the
                # device keeps per tensor must agree within the group (optimization.py:283-284 evaluates at state['step']
                # BEFORE incrementing it)
                if steps is None:
                    steps = f["steps"].tolist()
                taken = sorted(set(s for s, gid, fl in zip(steps, f["group_ids"], f["opt_flags"]) if fl and gid == gi))
                if len(taken) > 1:
                    raise NotImplementedError("fused BertAdam: %s is evaluated on the host from ONE step count per group, "
                                              "the tensors of group %d are at %s" % (type(sch).__name__, gi, taken))
                mult = float(sch.get_lr(taken[0] if taken else 0))
            rows += [float(g["lr"]), float(g["b1"]), float(g["b2"]), float(g["e"]), float(g["weight_decay"]),
                     float(g["max_grad_norm"]), float(code), float(getattr(sch, "warmup", 0.0)),
                     float(getattr(sch, "t_total", -1.0)), float(getattr(sch, "cycles", 0.0) or 0.0), mult]
            rows += self._extra_columns(g)
        return rows

    @staticmethod
    def _one_set_of_scalars(rows, f):
        """(lr, b1, b2, eps, weight_decay, max_grad_norm, warmup, t_total, schedule) for vb_bert_adam_step when the groups of
        `rows` differ in weight decay only -- one non-zero value, on exactly the tensors whose decay flag (tensor table, bit 1)
        was set when the tables were built -- and the schedule is warmup-linear or constant; else None."""
        g0 = rows[:GROUP_COLS]
        code, t_total = int(g0[6]), g0[8]
        if code == _HOST_SCHEDULE or not (code in (0, 1) or t_total < 0):
            return None
        decays = set()
        for gi in range(len(rows) // GROUP_COLS):
            r = rows[gi * GROUP_COLS:(gi + 1) * GROUP_COLS]
            if r[:4] != g0[:4] or r[5:9] != g0[5:9] or (r[4] > 0.0) != f["group_decays"][gi]:
                return None
            if r[4] > 0.0:
                decays.add(r[4])
        if len(decays) > 1:
            return None
        return (g0[0], g0[1], g0[2], g0[3], decays.pop() if decays else 0.0, g0[5], g0[7], t_total,
                1 if (code == 1 and t_total >= 0) else 0)

    def _touched_flags(self, f):
        """The reference's step() skips a parameter whose .grad is None -- no moment update, no weight decay
        (optimization.py:254-255): a head's unused tensors (cls.* under `flickr`, seq_relationship under `vqa_advanced`), the
        visual tables on a text-only batch, ...  Here every gradient is a view into the flat arena and always exists, so
        the backward pass records which parameters it wrote (ParameterArena.touched) and hands the optimizer KERNEL one
        flag per tensor; the kernel skips a tensor iff its flag is 0 and its gradient norm is 0.  Nothing is cached on the
        host between steps: under data parallelism the flags are all-reduced with the gradients
        (DataParallelGradSync.finish_step -> arena.touched_synced), so every rank takes the same decision every step."""
        a = f["arena"]
        synced = getattr(a, "touched_synced", None)
        if synced is not None:                                  # this step's flags, already combined over the ranks
            a.touched_synced = None
            return synced
        return a.touched_flags()

    @staticmethod
    def _carry_state(old, f):
        """moments and step counters follow their parameters by NAME from one fused state into a freshly built one."""
        a0, a1 = old["arena"], f["arena"]
        where = {n: (o, p.numel(), i) for i, (n, p, o) in enumerate(zip(a0.names, a0.params, a0.offsets))}
        steps0, steps1 = old["steps"].tolist(), f["steps"].tolist()
        for i, (n, p, o) in enumerate(zip(a1.names, a1.params, a1.offsets)):
            if n not in where or where[n][1] != p.numel():
                raise RuntimeError("visualbert_amd.BertAdam: parameter %r changed under a running optimizer" % n)
            o0, cnt, i0 = where[n]
            f["m"][o:o + cnt].copy_(old["m"][o0:o0 + cnt])
            f["v"][o:o + cnt].copy_(old["v"][o0:o0 + cnt])
            steps1[i] = steps0[i0]
        f["steps"].copy_(torch.tensor(steps1, dtype=torch.int32))

    def fused(self):
        f = self._fused
        if f is None or f["arena"] is not getattr(self.param_groups[0]["params"][0], "_vb_arena", None):
            old = f
            f = self._build()
            if old is not None and int(old["steps"].max()) > 0:
                # the model was moved / re-laid-out after training had started (TrainVisualBERTObjective._apply rebuilds the
                # arena): the moments and step counters follow their parameters by NAME instead of silently restarting
                self._carry_state(old, f)
        return f

    def add_param_group(self, param_group):
        """a group added after steps have been taken: the tables are rebuilt (the new tensors join with zero moments and a zero
        counter), every earlier parameter keeps its moments and its counter."""
        super(BertAdam, self).add_param_group(param_group)
        old = getattr(self, "_fused", None)
        if old is not None:
            self._fused = None
            if old["arena"] is getattr(self.param_groups[0]["params"][0], "_vb_arena", None):
                self._carry_state(old, self._build())

    def zero_grad(self, set_to_none=False):
        """one memset of the flat gradient arena; .grad stays a view into it (set_to_none is ignored on
        purpose: the kernels accumulate straight into these views)."""
        self.fused()["arena"].zero_grad()

    def get_lr(self):
        """one value per optimised tensor, in arena order: its own group's lr times its own group's schedule at its own step."""
        f = self.fused()
        steps = f["steps"].tolist()
        out = []
        for s, gid, fl in zip(steps, f["group_ids"], f["opt_flags"]):
            if fl:
                g = self.param_groups[gid]
                out.append(g["lr"] * g["schedule"].get_lr(s))
        return out

    def _upload_table(self, f, rows):
        """the device copy of the group table follows its host image; True when it had to be copied (first step, or a
        hyper-parameter was changed since the last upload)."""
        fresh = rows != f["gt_host"]
        if fresh:
            f["gt"].copy_(torch.tensor(rows, dtype=torch.float64))
            f["gt_host"] = rows
            self.table_uploads += 1
        return fresh

    def _launch(self, f, touched, rows):
        a = f["arena"]
        L = _lib.lib()
        one = self._one_set_of_scalars(rows, f)
        if one is not None:
            # every group shares one set of hyper-parameters the scalar entry can express (the reference's own training set-up,
            # models/model_wrapper.py:108-139: two groups that differ in weight decay only): no table, and the numbers of every
            # earlier release of this package, bit for bit
            rc = L.vb_bert_adam_step(_lib.ptr(a.data), _lib.ptr(a.grad), _lib.ptr(f["m"]), _lib.ptr(f["v"]),
                                     _lib.ptr(a.shadow), _lib.ptr(f["ct"]), f["nc"], _lib.ptr(f["tt"]), f["nt"],
                                     _lib.ptr(touched), _lib.ptr(f["norm2"]), _lib.ptr(f["steps"]), *one,
                                     _lib.stream_ptr())
            _lib.check(rc, "vb_bert_adam_step")
        else:
            fresh = self._upload_table(f, rows)
            # the library checks the tables' contents (group ids, schedule codes) only when asked to: it has to read them back
            rc = L.vb_bert_adam_step_groups(_lib.ptr(a.data), _lib.ptr(a.grad), _lib.ptr(f["m"]), _lib.ptr(f["v"]),
                                            _lib.ptr(a.shadow), _lib.ptr(f["ct"]), f["nc"], _lib.ptr(f["tt"]), f["nt"],
                                            _lib.ptr(touched), _lib.ptr(f["norm2"]), _lib.ptr(f["steps"]), _lib.ptr(f["gt"]),
                                            f["n_groups"], 1 if fresh else 0, _lib.stream_ptr())
            _lib.check(rc, "vb_bert_adam_step_groups")

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        f = self.fused()
        a = f["arena"]
        touched = self._touched_flags(f)
        self._launch(f, touched, self._group_rows(f))
        # the kernel refreshed the bf16 shadows of every optimised 2-D parameter
        shadowed = f.get("shadowed")
        if shadowed is None:                         # (the fused state -- and this list with it -- is rebuilt by load_state_dict)
            member = set()
            for group in self.param_groups:
                for p in group["params"]:
                    member.add(id(p))
            shadowed = f["shadowed"] = [p for p in a.params if p.dim() == 2 and id(p) in member]
        for p in shadowed:
            p._vb_shadow_ver = p._version
        a.refresh_transposed()                       # W^T copies for the next backward (one launch)
        ops.bump_x3_epoch()                          # split (bf16x3) images of the weights are re-made at their next use
        return loss

    # -- checkpoint compatibility: per-parameter {'step', 'next_m', 'next_v'} like the reference ------
    def state_dict(self):
        f = self.fused()
        a = f["arena"]
        steps = f["steps"].tolist()
        state = {}
        idx = {id(p): i for i, p in enumerate(a.params)}
        k = 0
        groups = []
        for group in self.param_groups:
            ids = []
            for p in group["params"]:
                i = idx[id(p)]
                o, n = a.offsets[i], p.numel()
                state[k] = {"step": steps[i], self._moment_keys[0]: f["m"][o:o + n].view(p.shape).clone(),
                            self._moment_keys[1]: f["v"][o:o + n].view(p.shape).clone()}
                ids.append(k)
                k += 1
            gd = {kk: vv for kk, vv in group.items() if kk not in ("params", "schedule")}
            gd["params"] = ids
            gd["schedule"] = _schedule_dict(group["schedule"])       # not the object and not a bare class name
            groups.append(gd)
        return dict(state=state, param_groups=groups)

    def load_state_dict(self, sd):
        # hyper-parameters and the schedule travel with the checkpoint, per group (saved as {"class", "warmup", "t_total",
        # "cycles"}, the schedule's attributes); a checkpoint written by the reference carries the schedule OBJECT of its own
        # module -- rebuilt here by class name.  A user schedule (a class this module does not know) stays as the group has it.
        for group, saved in zip(self.param_groups, sd.get("param_groups", [])):
            for k, v in saved.items():
                if k in ("params", "schedule"):
                    continue
                group[k] = v
            sch = saved.get("schedule")
            if sch is not None and not isinstance(sch, dict):
                sch = _schedule_dict(sch)
            if isinstance(sch, dict) and sch.get("class") in _SCHEDULE_CLASSES:
                group["schedule"] = _schedule_from_dict(sch)
        # the fused state caches the group ids and the device tables: rebuild it (the moments and counters are overwritten from
        # the checkpoint right below; the group table is re-made from the restored hyper-parameters at the next step)
        old = self._fused
        self._fused = None
        f = self.fused()
        if old is not None and old["m"].shape == f["m"].shape:
            # parameters the checkpoint does not mention keep the moments and counters they had (the reference's
            # Optimizer.load_state_dict replaces `state` wholesale only for the ids it lists; a partial checkpoint must not
            # silently zero the rest)
            f["m"].copy_(old["m"])
            f["v"].copy_(old["v"])
            f["steps"].copy_(old["steps"])
        a = f["arena"]
        idx = {id(p): i for i, p in enumerate(a.params)}
        steps = f["steps"].tolist()
        k = 0
        for group in self.param_groups:
            for p in group["params"]:
                st = sd["state"].get(k)
                if st is not None:
                    i = idx[id(p)]
                    o, n = a.offsets[i], p.numel()
                    f["m"][o:o + n].view(p.shape).copy_(st[self._moment_keys[0]])
                    f["v"][o:o + n].view(p.shape).copy_(st[self._moment_keys[1]])
                    steps[i] = int(st["step"])
                k += 1
        f["steps"].copy_(torch.tensor(steps, dtype=torch.int32))


class Lamb(BertAdam):
    """LAMB for large-batch training (You et al., "Large Batch Optimization for Deep Learning", NVLAMB conventions), as one fused
    multi-tensor kernel sequence over the parameter arena (vb_lamb_step_groups).  Per step: every gradient is scaled by
    min(1, max_grad_norm / global norm) -- ONE norm over all optimised tensors of all groups, each group applying its own
    max_grad_norm to it; Adam moments with (bias_correction) or without division by 1 - beta^t; update u = m / (sqrt(v) + e) +
    weight_decay * p; and every tensor moves by lr * schedule(step) * r * u with its own trust ratio r = ||p|| / ||u|| (1 when
    either norm is 0, and 1 for a tensor without weight decay unless always_adapt).

    Every key is per parameter group, schedules (objects, or user subclasses evaluated on the host) and the `.grad is None` rule
    work as in BertAdam, and so do zero_grad, get_lr (lr x schedule; the trust ratio lives on the device), add_param_group, the
    carry-over of state when the arena is rebuilt, and the hand-over of `touched` flags under DataParallelGradSync.  Gradients are
    only read.  state_dict keeps {'step', 'exp_avg', 'exp_avg_sq'} per parameter and each group's hyper-parameters with its
    schedule as a dict."""

    _group_cols = LAMB_GROUP_COLS
    _moment_keys = ("exp_avg", "exp_avg_sq")

    def __init__(self, params, lr=1e-3, warmup=-1, t_total=-1, schedule='warmup_linear', b1=0.9, b2=0.999, e=1e-6,
                 weight_decay=0.01, max_grad_norm=1.0, bias_correction=True, always_adapt=False):
        super(Lamb, self).__init__(params, lr=lr, warmup=warmup, t_total=t_total, schedule=schedule, b1=b1, b2=b2, e=e,
                                   weight_decay=weight_decay, max_grad_norm=max_grad_norm, bias_correction=bias_correction,
                                   always_adapt=always_adapt)

    def _extra_defaults(self, kwargs):
        return dict(bias_correction=bool(kwargs["bias_correction"]), always_adapt=bool(kwargs["always_adapt"]))

    def _extra_columns(self, group):
        return [1.0 if group["bias_correction"] else 0.0, 1.0 if group["always_adapt"] else 0.0]

    def _ws_floats(self, nt, nc):
        return int(_lib.lib().vb_lamb_ws_floats(nt, nc))

    def _launch(self, f, touched, rows):
        a = f["arena"]
        fresh = self._upload_table(f, rows)
        # as in BertAdam: the library reads the tables back to check them only when they are new
        rc = _lib.lib().vb_lamb_step_groups(_lib.ptr(a.data), _lib.ptr(a.grad), _lib.ptr(f["m"]), _lib.ptr(f["v"]),
                                            _lib.ptr(a.shadow), _lib.ptr(f["ct"]), f["nc"], _lib.ptr(f["tt"]), f["nt"],
                                            _lib.ptr(touched), _lib.ptr(f["norm2"]), _lib.ptr(f["steps"]), _lib.ptr(f["gt"]),
                                            f["n_groups"], 1 if fresh else 0, _lib.stream_ptr())
        _lib.check(rc, "vb_lamb_step_groups")
