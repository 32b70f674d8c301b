"""Recurrence prior on the resident stream: "what did (s, r) connect to before, how often, how recently" under the observed
protocol -- the same histories, the same filter lists, the same tie rule as the model's own numbers.

Two uses.  `evaluate` / `topk` are the MODEL-FREE baseline: uniform logits through the mix kernel, then the rank / top-k
kernels and filter lists of RENet.evaluate_forecast / forecast_topk, in their result layouts -- a protocol-matched yardstick,
to be reported with its alpha and half_life.  And the `prior=` keyword of RENet.evaluate_observed, evaluate_forecast,
forecast_scores, forecast_topk and evaluate_online: every score matrix goes through ONE renet_recurrence_mix_rows launch
between the score GEMM and the rank / top-k kernel,

    out[o] = log((1 - a) softmax(logits)[o] + a w[o] / W),   w[o] = sum over the facts (ent, rel, o, t' < as_of) of
                                                                     2^(-(t - t') / half_life),   W = sum of w

with a = alpha where the pair (ent, rel) has history before as_of and 0 where it has none: there the prior abstains and
the row is log_softmax(logits).  The as_of that cuts the prior is the one that cuts the model's histories: a stale-history
query gets a stale prior, nothing at or after as_of is read.  alpha = 0 is log_softmax of the logits: its ranks equal the
unmixed ones except where the subtraction of the row's logsumexp rounds two logits together.

The statistic is read from the resident PAIR TABLES (gpu_builder.ObservedStore.pair_tables; host statement
preprocess.PairIndex), built on first use and carried through ObservedStream.observe() by renet_pair_append.

TRAINING through the mix.  A CopyGate is the learned form of the prior: one gate per (side, relation), a = sigmoid(logit),
accepted wherever `prior=` is (one renet_recurrence_mix_rows_gated launch in the scalar entry's place).  For a row with gold
column g, p = softmax(logits), q = w[g] / W and m = (1 - a) p_g + a q, the loss L = -log m has
    dL/dlogits[c] = s (p_c - [c == g]),  s = (1 - a) p_g / m in [0, 1],      dL/da = (p_g - q) / m
-- the CE gradient times one scalar per row, and of the prior only the gold column's mass: CopyRows gathers (a, q, W) of a
merged training batch with two renet_recurrence_gold_rows launches, RENet.loss_prepared_both(prep, copy=) and
RENet.learn_observed(..., prior=, gate_optimizer=) train the model (and the gate) through the mix, fit_gate fits the gate
alone.  A step with copy= is not in the C launch list (csrc/step.cpp): it pays the autograd path's host enqueue.  Numbers
with a LEARNED gate are a protocol of their own: comparable only with numbers of the same protocol and the same fitting data.

A LEARNED HALF-LIFE.  CopyGate(learn_half_life=True) also learns HOW RECENT a fact must be to count: one decay per (side,
relation), rate = exp(log_rate) = 1 / half_life in the stream's timestamp units, initialised from half_life.  Every row takes
its own rate (renet_recurrence_mix_rows_decay / renet_recurrence_gold_rows_decay in the gated / gold entries' places).  With
the lag D = t - t' and w = 2^(-D rate):  G = sum over gold's facts of w, W = sum over all, GD / WD the same sums of D w,
    q = G / W,   dq/drate = -ln2 (GD W - G WD) / W^2 = -ln2 q (E_gold[D] - E_all[D]),   dL/dq = -a / m = -a exp(L)
-- the gold kernel returns dq beside q, the head Functions return dL/dq from their row losses (the CE writers are untouched),
and the product reaches log_rate through the gates' deterministic segmented add: d log_rate[k] = rate_k * sum over the rows of
k.  log_rate is a gate parameter: gate_optimizer steps it, it stays out of the model's clip norm.  Numbers with learned
parameters are a protocol of their own: report the INITIAL alpha and half_life, the fitting split, steps and learning rate.

EVENTS.  The event entries (RENet.evaluate_events_observed, predict_events_observed, observed_event_scores, forecast_events)
rank a (relation, entity) PAIR among R * N_ent candidates; their `prior=` keyword mixes the JOINT statistic into the joint
log-probabilities J of a history (a "group": the given entity e, t, as_of) with one renet_joint_mix_rows call per sub-block,
between renet_joint_row_offsets and the rank / top-k launches:

    M[r, c] = log((1 - a) exp(J[r, c]) + a w[r, c] / W),   w[r, c] = sum over the facts (e, r, c, t' < as_of) of
                                                                      2^(-(t - t') / half_life),   W = sum of ALL w of e

W is entity-wide -- "s does again what it did before, with whom it did it", whatever the relation -- so exp(M) is a
distribution over the pairs as exp(J) is, and a = alpha where e has any history before as_of, else 0.  A RecurrencePrior is
taken as it is; a CopyGate(per_relation=False) as its side's single gate, read to the host once per call; a per-relation
CopyGate is refused: with the relation open, a gate per relation does not give a normalised joint.  `evaluate_events` is the
MODEL-FREE baseline in evaluate_events_observed's layout (the uniform joint through the same mix entry, groups, filter lists
and tie rule).  The baseline's and the mixed event numbers go beside event numbers of the SAME protocol only, and with their
alpha and half_life.  `topk_events` is the baseline's top-k in predict_events_observed's layout, through that entry's own tail.

TRAINING THROUGH THE JOINT MIX.  The training loss of a row is the unmixed event loss already, CE_e + CE_r = -J[r*, g]; with
EventCopyRows (RENet.loss_prepared_both(prep, event_copy=), RENet.learn_observed(event_prior=, gate_optimizer=)) it is

    L = -log((1 - a) p_g pr + a q) = -M[r*, g],     q = G / W from renet_joint_gold_rows(_decay), W entity-wide as above

and both heads receive their plain CE gradient times ONE scalar per row, s = (1 - a) p_g pr / m (ops.DualHeadCEFn, event_a /
event_q; renet_joint_mix_ce(_planes) is renet_mix_ce(_planes) with lp = log pr added to the gold logit).  a is a
RecurrencePrior's alpha or the side's single gate of a CopyGate(per_relation=False), with autograd; a gate that learns its
decay gets dq from the decay entry.  fit_event_gate fits such a gate with the model frozen: it PRODUCES the two numbers
event_scalars() reads.  Numbers with a fitted event gate are a protocol of their own: report them with the INITIAL alpha and
half_life, the fitting split, steps and learning rate.

Not covered: rollout (generated facts in a prior are a protocol question of their own; generate_events_observed and
evaluate_rollout take no prior: generation stays the model's own), a learned per-relation
gate for events, evaluate_online with an event prior, the C launch list for steps with a prior, fusing the mix into
renet_joint_row_offsets or the rank kernel (measured first: profiles/event_prior.md), a
relation-free term, a per-relation decay for events, bf16-storage mode, data-parallel gate gradients."""
import math

import numpy as np
import torch

import filter_index as FI
import graph as G
import renet_hip as K

SETTINGS = ('raw', 'filtered', 'time_filtered')
SIDES = {'ob': 0, 'sub': 1}              # the side predicted -> the role of the GIVEN entity (0: subject runs, 1: object runs)


class RecurrencePrior(object):
    """alpha: the weight of the recurrence term, 0 <= alpha < 1.  half_life: in the stream's raw timestamp units, the age
    at which a fact counts half; None: frequency only.  The kernel takes both as fp32: `alpha` and `inv_half_life` here are
    the rounded values, which the host statement (preprocess.PairIndex.prior_rows(..., inv_half_life=)) uses as they stand."""

    def __init__(self, alpha, half_life=None):
        alpha = float(np.float32(alpha))
        if not 0.0 <= alpha < 1.0:
            raise ValueError('alpha must lie in [0, 1)')
        if half_life is not None and not float(half_life) > 0.0:
            raise ValueError('half_life must be positive (None: frequency only)')
        self.alpha = alpha
        self.half_life = None if half_life is None else float(half_life)
        self.inv_half_life = 0.0 if half_life is None else float(np.float32(1.0 / float(half_life)))

    def __repr__(self):
        return 'RecurrencePrior(alpha=%g, half_life=%r)' % (self.alpha, self.half_life)


class _GateRowsFn(torch.autograd.Function):
    """out[i] = table[index[i]] for the flat gate table [T]; backward: the rows' gradients summed per gate by the project's
    segmented add over a plan sorted by (side, relation) -- a fixed order, no floating-point atomics, the same bits from run
    to run (index_add_ gives neither)."""

    @staticmethod
    def forward(ctx, table, index, plan):
        ctx.plan, ctx.size = plan, table.numel()
        return table[index]

    @staticmethod
    def backward(ctx, g):
        src = torch.zeros(g.numel(), 4, device=g.device, dtype=torch.float32)      # (the segmented add takes float4 rows)
        src[:, 0] = g
        dst = torch.zeros(ctx.size, 4, device=g.device, dtype=torch.float32)
        K.segment_add(src, ctx.plan, dst)
        return dst[:, 0].contiguous(), None, None


class _PermuteFn(torch.autograd.Function):
    """out = x[perm] for a PERMUTATION perm; backward scatters without accumulation: one writer per element."""

    @staticmethod
    def forward(ctx, x, perm):
        ctx.perm = perm
        return x[perm]

    @staticmethod
    def backward(ctx, g):
        out = torch.empty_like(g)
        out[ctx.perm] = g
        return out, None


class _DecayQFn(torch.autograd.Function):
    """q as a function of the per-row decay: forward returns the gold kernel's q (its bits), backward g * dq with the
    kernel's dq = d q / d rate -- an elementwise product, one writer per row."""

    @staticmethod
    def forward(ctx, rate, q, dq):
        ctx.save_for_backward(dq)
        return q.clone()

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


A_MAX = 1.0 - 2.0 ** -24                  # the largest fp32 below 1: a gate never reaches 1, whatever its logit


class CopyGate(torch.nn.Module):
    """The LEARNED recurrence prior: one gate per side and relation, a = sigmoid(logit).  logit: fp32 [2, num_rels] (row 0 the
    'ob' side -- objects of (s, r, ?) --, row 1 the 'sub' side), or [2, 1] with per_relation=False; initialised to
    logit(alpha).  half_life as RecurrencePrior's, fixed -- or, with learn_half_life=True, LEARNED: a second parameter
    log_rate, fp32 in logit's layout, rate = exp(log_rate) = 1 / half_life per (side, relation), initialised to
    log(1 / half_life) (half_life is then required); every row is mixed with its own rate and the loss reaches log_rate
    through q (see the module's text).  Accepted wherever `prior=` takes a RecurrencePrior; trained by
    RENet.learn_observed(prior=gate, gate_optimizer=) and fit_gate.  state_dict() holds `logit`, and `log_rate` with
    learn_half_life=True only."""

    def __init__(self, num_rels, alpha=0.3, half_life=None, per_relation=True, learn_half_life=False):
        super(CopyGate, self).__init__()
        alpha = float(alpha)
        if not 0.0 < alpha < 1.0:
            raise ValueError('alpha must lie in (0, 1): it initialises logit = log(alpha / (1 - alpha))')
        if half_life is not None and not float(half_life) > 0.0:
            raise ValueError('half_life must be positive (None: frequency only)')
        if learn_half_life and half_life is None:
            raise ValueError('learn_half_life=True needs half_life: it initialises log_rate = log(1 / half_life)')
        self.num_rels, self.per_relation = int(num_rels), bool(per_relation)
        if self.num_rels < 1:
            raise ValueError('num_rels must be positive')
        self.half_life = None if half_life is None else float(half_life)
        self.inv_half_life = 0.0 if half_life is None else float(np.float32(1.0 / float(half_life)))
        width = self.num_rels if self.per_relation else 1
        self.logit = torch.nn.Parameter(torch.full((2, width), math.log(alpha / (1.0 - alpha)), dtype=torch.float32))
        self.learn_half_life = bool(learn_half_life)
        if self.learn_half_life:
            self.log_rate = torch.nn.Parameter(torch.full((2, width), math.log(1.0 / float(half_life)), dtype=torch.float32))
        self._checked_version = self._checked_rate = None

    def __repr__(self):
        return 'CopyGate(num_rels=%d, half_life=%r, per_relation=%r%s)' % (
            self.num_rels, self.half_life, self.per_relation, ', learn_half_life=True' if self.learn_half_life else '')

    def table(self):
        """The gates [2, width] = sigmoid(logit), kept below 1."""
        return torch.sigmoid(self.logit).clamp(max=A_MAX)

    def check(self):
        """Refuses a gate table that is not inside [0, 1) (a NaN logit) -- one small read-back per change of the parameter,
        so that the gated mix kernel, which cannot check device memory, is never launched on one."""
        key = (self.logit._version, self.logit.data_ptr())
        if self._checked_version != key:
            tab = self.table().detach()
            if not bool(((tab >= 0) & (tab < 1)).all()):
                raise ValueError('CopyGate: a gate outside [0, 1) (non-finite logit?)')
            self._checked_version = key
        if self.learn_half_life:
            key = (self.log_rate._version, self.log_rate.data_ptr())
            if self._checked_rate != key:
                rate = self.rate_table().detach()
                if not bool(((rate >= 0) & (rate < float('inf'))).all()):
                    raise ValueError('CopyGate: a decay that is negative or not finite (non-finite log_rate?)')
                self._checked_rate = key
        return self

    def rate_table(self):
        """The learned decays [2, width] = exp(log_rate), 1 / half_life per (side, relation); learn_half_life=True only."""
        if not self.learn_half_life:
            raise ValueError('CopyGate: rate_table() needs learn_half_life=True (the fixed decay is inv_half_life)')
        return torch.exp(self.log_rate)

    def half_lives(self):
        """The learned half-lives, a host float64 array [2, width] = 1 / rate_table(): for reports."""
        return 1.0 / self.rate_table().detach().double().cpu().numpy()

    def index(self, side, rel):
        """The flat index into table() of the rows of `side` with relations rel (host array or device tensor)."""
        if side not in SIDES:
            raise ValueError("side must be 'ob' or 'sub'")
        width = self.logit.shape[1]
        if isinstance(rel, torch.Tensor):
            r = rel.long()
            if self.per_relation and r.numel() and (int(r.min()) < 0 or int(r.max()) >= self.num_rels):
                raise ValueError('relation outside [0, num_rels)')
            return (r if self.per_relation else torch.zeros_like(r)) + SIDES[side] * width
        r = np.asarray(rel, dtype=np.int64).reshape(-1)
        if self.per_relation and len(r) and (r.min() < 0 or r.max() >= self.num_rels):
            raise ValueError('relation outside [0, num_rels)')
        return (r if self.per_relation else np.zeros_like(r)) + SIDES[side] * width

    def rows_at(self, index):
        """The gates at the flat table indices `index` (host int array), a device tensor with autograd: its gradient reaches
        `logit` through a deterministic segmented add."""
        return self._rows_of(self.table().reshape(-1), self.logit, index)

    def rate_rows_at(self, index):
        """rows_at for the learned decays: rate_table() at the flat indices `index`, its gradient reaching `log_rate` through
        the same plan and the same deterministic segmented add."""
        return self._rows_of(self.rate_table().reshape(-1), self.log_rate, index)

    def rate_rows(self, side, rel):
        """rows for the learned decays: the per-row rate of the rows of `side` with relations rel."""
        if isinstance(rel, torch.Tensor):
            if not (torch.is_grad_enabled() and self.log_rate.requires_grad):
                return self.rate_table().detach().reshape(-1)[self.index(side, rel)]
            rel = rel.cpu().numpy()
        return self.rate_rows_at(self.index(side, rel))

    def _rows_of(self, flat, param, index):
        dev = param.device
        index = np.ascontiguousarray(index, dtype=np.int64)
        idx_dev = torch.from_numpy(index).to(dev)
        if not (torch.is_grad_enabled() and param.requires_grad) or len(index) == 0:
            return flat.detach()[idx_dev]
        hp, plan = G.SegPlan.host(index), G.SegPlan()
        plan.order, plan.seg_ptr, plan.target = (G.h2d(np.ascontiguousarray(a, dtype=np.int32), dev)
                                                 for a in (hp.order, hp.seg_ptr, hp.target))
        plan.num_segments = hp.num_segments
        return _GateRowsFn.apply(flat, idx_dev, plan)

    def rows(self, side, rel):
        """The per-row gate of the rows of `side` ('ob' / 'sub') with relations rel, a device tensor with autograd."""
        if isinstance(rel, torch.Tensor):
            if not (torch.is_grad_enabled() and self.logit.requires_grad):
                return self.table().detach().reshape(-1)[self.index(side, rel)]
            rel = rel.cpu().numpy()
        return self.rows_at(self.index(side, rel))


class QueryRows(object):
    """What the mix kernel needs of the rows of a resident store, as int32 device tensors: per role the given entity (-1:
    absent), the relation, t and as_of.  store: a gpu_builder.ObservedStore with the stream positions idx (as_of = t) or a
    gpu_builder.QueryStore (idx indexes its queries)."""

    def __init__(self, store, idx):
        dev = store.device
        pos = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(dev)
        self.base = getattr(store, 'base', store)
        self.tables = store.pair_tables()
        if 'as_of' in store.t:                                          # a QueryStore: an absent side gathers entity 0 there
            ent = torch.where(store.present, torch.stack((store.t['q_s'], store.t['q_o'])), -1).to(torch.int32)
            self.ent = (ent[0][pos].contiguous(), ent[1][pos].contiguous())
            self.t, self.as_of = store.t['t'][pos].contiguous(), store.t['as_of'][pos].contiguous()
        else:
            self.ent = (store.t['q_s'][pos], store.t['q_o'][pos])
            self.t = torch.from_numpy(np.ascontiguousarray(store.quads[idx, 3], dtype=np.int32)).to(dev)
            self.as_of = self.t
        self.rel = store.t['q_r'][pos].contiguous()

    def mix(self, prior, name, logits, c=0, d=None, want_stats=False):
        """The rows [c, d) of side `name` ('ob': objects of (s, r, ?), 'sub': subjects of (?, r, o)) through one
        renet_recurrence_mix_rows launch; logits [d - c, N_ent] or None (uniform)."""
        role = SIDES[name]
        d = int(self.rel.numel()) if d is None else d
        t = self.base.t
        if isinstance(prior, CopyGate):                                 # one gate per row: the gated entry
            width = prior.logit.shape[1]
            with torch.no_grad():
                tab = prior.check().table().reshape(-1)
                rel = self.rel[c:d].long()
                if width > 1:
                    rel = rel.clamp(0, width - 1)        # (a relation the gate does not know reads a neighbour's gate, never memory)
                else:
                    rel = torch.zeros_like(rel)
                a_row = tab[rel + role * width].contiguous()
                if prior.learn_half_life:                               # one decay per row as well: gathered as a_row is
                    ihl_row = prior.rate_table().reshape(-1)[rel + role * width].contiguous()
            if prior.learn_half_life:
                return K.recurrence_mix_rows_decay(self.ent[role][c:d], self.rel[c:d], self.t[c:d], self.as_of[c:d],
                                                   self.tables[role], t['ent_ptr%d' % role], t['snap_ptr%d' % role],
                                                   self.base.num_ent, logits, a_row, ihl_row, num_cols=self.base.num_ent,
                                                   want_stats=want_stats, check=False)
            return K.recurrence_mix_rows_gated(self.ent[role][c:d], self.rel[c:d], self.t[c:d], self.as_of[c:d],
                                               self.tables[role], t['ent_ptr%d' % role], t['snap_ptr%d' % role],
                                               self.base.num_ent, logits, a_row, prior.inv_half_life,
                                               num_cols=self.base.num_ent, want_stats=want_stats, check=False)
        return K.recurrence_mix_rows(self.ent[role][c:d], self.rel[c:d], self.t[c:d], self.as_of[c:d], self.tables[role],
                                     t['ent_ptr%d' % role], t['snap_ptr%d' % role], self.base.num_ent, logits, prior.alpha,
                                     prior.inv_half_life, num_cols=self.base.num_ent, want_stats=want_stats)


def _checked(prior):
    if not isinstance(prior, (RecurrencePrior, CopyGate)):
        raise ValueError('prior must be a recurrence.RecurrencePrior or a recurrence.CopyGate')
    return prior


def event_scalars(prior):
    """({'ob': a, 'sub': a}, {'ob': inv_half_life, 'sub': inv_half_life}): the scalar weight and decay of the JOINT mix per
    direction.  A RecurrencePrior gives its alpha and inv_half_life for both; a CopyGate(per_relation=False) its side's single
    gate and -- with learn_half_life=True -- its side's single learned rate (checked, then read to the host: ONE small copy per
    call for both).  A per-relation CopyGate is refused: the joint mix takes ONE gate and ONE decay per history."""
    _checked(prior)
    if not isinstance(prior, CopyGate):
        return {name: prior.alpha for name in SIDES}, {name: prior.inv_half_life for name in SIDES}
    if prior.per_relation:
        raise ValueError('the event entries take a RecurrencePrior or a CopyGate(per_relation=False), not a per-relation gate: '
                         'with the relation open, a gate per relation does not give a normalised joint')
    tab = prior.check().table().detach().reshape(-1)                                # [2]: the 'ob' gate, the 'sub' gate
    if not prior.learn_half_life:
        tab = tab.cpu().numpy()
        return ({name: float(np.float32(tab[row])) for name, row in SIDES.items()},
                {name: prior.inv_half_life for name in SIDES})
    tab = torch.stack((tab, prior.rate_table().detach().reshape(-1))).cpu().numpy()  # [2, 2]: the gates, the rates
    return tuple({name: float(np.float32(row[k])) for name, k in SIDES.items()} for row in tab)


def event_alphas(prior):
    """event_scalars(prior)[0]: {'ob': a, 'sub': a}."""
    return event_scalars(prior)[0]


def event_alpha(prior, name):
    """event_alphas(prior)[name] for the direction name ('ob': pairs (r, o) of a subject, 'sub': pairs (r, s) of an object)."""
    if name not in SIDES:
        raise ValueError("direction must be 'ob' or 'sub'")
    return event_alphas(prior)[name]


class EventMix(object):
    """What the `prior=` keyword of the event entries carries through one call: the two directions' alpha (event_alphas, read
    once) and inv_half_life (one per direction: a gate that learns its decay has one rate per side), and -- from the first
    groups() on -- the base store whose pair tables are read."""

    def __init__(self, prior):
        self.alpha, self.inv_half_life = event_scalars(prior)
        self.base = None

    def groups(self, store, ent, t, first):
        """(ent, t, as_of) of the groups of one direction of a chunk, int32 device [G]: ent, t host arrays; first [G] the store
        position whose history window is the group's -- its as_of on a QueryStore, the group's own t on an ObservedStore."""
        dev = store.device
        if self.base is None:
            self.base, self.tables = getattr(store, 'base', store), store.pair_tables()
        et = torch.from_numpy(np.ascontiguousarray(np.stack((ent, t)), dtype=np.int32)).to(dev)
        if 'as_of' in store.t:
            as_of = store.t['as_of'][torch.from_numpy(np.ascontiguousarray(first, dtype=np.int64)).to(dev)].contiguous()
        else:
            as_of = et[1]
        return et[0], et[1], as_of

    def apply(self, name, block, off, q, g0=0, g1=None, mass=None):
        """ONE renet_joint_mix_rows call on the sub-block (block [(g1 - g0) * R, C], off) of the groups [g0, g1) of direction
        `name`, in place; q: groups()' triple of the whole direction.  -> mass."""
        g1 = int(q[0].numel()) if g1 is None else g1
        role, t = SIDES[name], self.base.t
        return K.joint_mix_rows(block, block.shape[0] // max(g1 - g0, 1), off, q[0][g0:g1], q[1][g0:g1], q[2][g0:g1],
                                self.tables[role], t['ent_ptr%d' % role], t['snap_ptr%d' % role], self.base.num_ent,
                                self.alpha[name], self.inv_half_life[name], mass=mass)


class CopyRows(object):
    """(a_row, q_row, W) of ONE merged training batch, for RENet.loss_prepared_both(prep, copy=): the positions idx of the
    resident store `store` (a gpu_builder.ObservedStore; as_of = t: no fact of the query's own timestamp is read) under
    `prior` (RecurrencePrior: a = alpha; CopyGate: a = its gate of (side, relation), with autograd; a gate that learns its
    decay: renet_recurrence_gold_rows_decay with the rows' own rates, and q with autograd -- its backward hands g * dq to the
    per-row rates).  Two renet_recurrence_gold_rows launches, one per role -- sequence i < n of the merged batch is position i's 'ob' direction
    (given s, gold o), sequence n + i its 'sub' direction (given o, gold s) --, a zeroed where the prior abstains (W = 0), and
    in batch() one gather through the builder's perm (sorted position -> sequence) into the batch's row order."""

    def __init__(self, store, idx, prior):
        _checked(prior)
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        rows = QueryRows(store, idx)
        base, n = rows.base, len(idx)
        learned = isinstance(prior, CopyGate) and prior.learn_half_life
        if isinstance(prior, CopyGate):
            rel = store.quads[idx, 1]
            index = np.concatenate((prior.index('ob', rel), prior.index('sub', rel)))
            prior.check()
        if learned:
            rate = prior.rate_rows_at(index)                            # [2n], with autograd when log_rate learns
            ihl = rate.detach().contiguous()
        q, w, dq = [], [], []
        for role in (0, 1):
            args = (rows.ent[role], rows.rel, rows.t, rows.as_of, rows.ent[1 - role], rows.tables[role],
                    base.t['ent_ptr%d' % role], base.t['snap_ptr%d' % role], base.num_ent, base.num_ent)
            if learned:
                qq, ww, dd = K.recurrence_gold_rows_decay(*args, ihl[role * n:(role + 1) * n])
                dq.append(dd)
            else:
                qq, ww = K.recurrence_gold_rows(*args, prior.inv_half_life)
            q.append(qq)
            w.append(ww)
        self.n = n
        self.q_seq, self.W_seq = torch.cat(q), torch.cat(w)
        if learned and rate.requires_grad:
            self.q_seq = _DecayQFn.apply(rate, self.q_seq, torch.cat(dq))
        if isinstance(prior, CopyGate):
            a = prior.rows_at(index)
        else:
            a = torch.full((2 * n,), prior.alpha, device=self.q_seq.device, dtype=torch.float32)
        self.a_seq = torch.where(self.W_seq > 0, a, torch.zeros_like(a))

    def batch(self, prep):
        """-> (a_row, q_row, W) in the row order of the PreparedBatch prep built from the same positions."""
        if prep.b != 2 * self.n:
            raise ValueError('CopyRows: the batch does not hold the two directions of these positions')
        perm = prep.g._v['perm'][:prep.b].long()
        a = _PermuteFn.apply(self.a_seq, perm) if self.a_seq.requires_grad else self.a_seq[perm]
        q = _PermuteFn.apply(self.q_seq, perm) if self.q_seq.requires_grad else self.q_seq[perm]
        return a, q, self.W_seq[perm]


def _event_gate(prior):
    """prior checked for the EVENT loss: a RecurrencePrior, or a CopyGate(per_relation=False) (event_scalars' refusal)."""
    _checked(prior)
    if isinstance(prior, CopyGate):
        if prior.per_relation:
            raise ValueError('the event entries take a RecurrencePrior or a CopyGate(per_relation=False), not a per-relation '
                             'gate: with the relation open, a gate per relation does not give a normalised joint')
        prior.check()
    return prior


class EventCopyRows(object):
    """The event twin of CopyRows: (a_row, q_row, W) of ONE merged training batch for RENet.loss_prepared_both(prep,
    event_copy=), the loss through the JOINT mix of renet_joint_mix_rows.  Sequence i < n is position i's 'ob' direction (given
    s, gold pair (r, o)), sequence n + i its 'sub' direction (given o, gold pair (r, s)); as_of = t.  Two renet_joint_gold_rows
    launches, one per role: q = G / W with the ENTITY-WIDE W (every relation), not CopyRows' per-(s, r) one.  a is a
    RecurrencePrior's alpha, or the side's single gate of a CopyGate(per_relation=False), WITH autograd (rows_at with the
    side's one index: its gradient reaches `logit` through the deterministic segmented add); zeroed where W = 0.  A gate that
    learns its decay: renet_joint_gold_rows_decay with the side's rate on every row, and q with autograd (_DecayQFn).  A
    per-relation gate is refused (event_scalars' message)."""

    def __init__(self, store, idx, prior):
        _event_gate(prior)
        idx = np.asarray(idx, dtype=np.int64).reshape(-1)
        rows = QueryRows(store, idx)
        base, n = rows.base, len(idx)
        gate = isinstance(prior, CopyGate)
        learned = gate and prior.learn_half_life
        if gate:
            index = np.concatenate((np.full(n, SIDES['ob'], dtype=np.int64), np.full(n, SIDES['sub'], dtype=np.int64)))
        if learned:
            rate = prior.rate_rows_at(index)                            # [2n], with autograd when log_rate learns
            ihl = rate.detach().contiguous()
        q, w, dq = [], [], []
        for role in (0, 1):
            args = (rows.ent[role], rows.rel, rows.t, rows.as_of, rows.ent[1 - role], rows.tables[role],
                    base.t['ent_ptr%d' % role], base.t['snap_ptr%d' % role], base.num_ent, base.num_rels, base.num_ent)
            if learned:
                qq, ww, dd = K.joint_gold_rows_decay(*args, ihl[role * n:(role + 1) * n])
                dq.append(dd)
            else:
                qq, ww = K.joint_gold_rows(*args, prior.inv_half_life)
            q.append(qq)
            w.append(ww)
        self.n = n
        self.q_seq, self.W_seq = torch.cat(q), torch.cat(w)
        if learned and rate.requires_grad:
            self.q_seq = _DecayQFn.apply(rate, self.q_seq, torch.cat(dq))
        if gate:
            a = prior.rows_at(index)
        else:
            a = torch.full((2 * n,), prior.alpha, device=self.q_seq.device, dtype=torch.float32)
        self.a_seq = torch.where(self.W_seq > 0, a, torch.zeros_like(a))

    batch = CopyRows.batch


def fit_event_gate(model, obs, idx, gate, optimizer, steps=1, max_batch=4096):
    """fit_gate for EVENTS, the model FROZEN: `steps` optimizer steps of the CopyGate(per_relation=False) `gate` on the joint
    loss -log((1 - a) p(o | s, r) p(r | s) + a q) of the stream positions idx, both directions.  Per step and per batch of
    max_batch positions the entity scores and the relation logits of the gold rows are computed under no_grad as
    evaluate_observed(relation=True) computes them (eval mode); the relation head's row loss gives lp, renet_joint_mix_ce
    takes the entity scores with dlogits = NULL -- only d_a and d_q flow --, and the gradient of the MEAN joint loss over all
    rows of both directions is accumulated before ONE optimizer.step().  -> the mean joint loss per step (Python floats,
    before that step's update).  The model's parameters and mode are left as found."""
    import model as M
    import ops
    if not isinstance(gate, CopyGate):
        raise ValueError('fit_event_gate fits a recurrence.CopyGate(per_relation=False)')
    _event_gate(gate)
    store = M._observed_store(obs)
    idx = M._observed_positions(store, idx)
    max_batch = max(1, int(max_batch))
    n = len(idx)
    dev = gate.logit.device
    was_training = model.training
    model.eval()
    out = []
    try:
        for _ in range(int(steps)):
            optimizer.zero_grad()
            total = torch.zeros((), device=dev)
            with torch.no_grad():
                cuts = M._observed_cuts(M._observed_chunks(model, store, idx, True), max_batch)
            while True:
                with torch.no_grad():
                    cut = next(cuts, None)
                if cut is None:
                    break
                c, d, (feat_ob, feat_sub, featr_ob, featr_sub) = cut
                part = idx[c:d]
                rows = EventCopyRows(store, part, gate)
                m = len(part)
                rel = rows_rel(store, part)
                for k, (feat, featr, gold) in enumerate(((feat_ob, featr_ob, rows_gold(store, part, 'ob')),
                                                         (feat_sub, featr_sub, rows_gold(store, part, 'sub')))):
                    with torch.no_grad():
                        pred = M._linear_eval(model.linear, feat)
                        lp = -K.softmax_ce(M._linear_eval(model.linear_r, featr), rel, 1.0, False)
                    a, q = rows.a_seq[k * m:(k + 1) * m], rows.q_seq[k * m:(k + 1) * m]
                    row_loss, d_a, _ = K.joint_mix_ce(pred, gold, a.detach().contiguous(), q.detach().contiguous(), lp,
                                                      1.0 / (2 * n), False)
                    if a.requires_grad:
                        a.backward(d_a, retain_graph=True)
                    if q.requires_grad:                                  # (a learned decay: dL/dq = -a / m = -a exp(L))
                        q.backward(ops.copy_q_grad(a.detach(), row_loss, 1.0 / (2 * n)), retain_graph=True)
                    total = total + row_loss.sum() / (2 * n)
            optimizer.step()
            out.append(total)
    finally:
        model.train(was_training)
    return [float(x) for x in torch.stack(out).cpu()] if out else []


def rows_rel(store, idx):
    """The relation (int32 device [n]) of the stream positions idx: the gold class of the relation head, both directions."""
    pos = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(store.device)
    return store.t['q_r'][pos].contiguous()


def fit_gate(model, obs, idx, gate, optimizer, steps=1, max_batch=4096):
    """"Fitting alpha" with the model FROZEN: `steps` optimizer steps of the CopyGate `gate` on the stream positions idx of
    the resident stream obs.  Per step and per batch of max_batch positions the scores are computed under no_grad as
    RENet.observed_scores computes them (eval mode), renet_mix_ce takes them with dlogits = NULL -- only d_a flows --, and the
    gate's gradient of the MEAN mixed loss over all rows of both directions is accumulated before ONE optimizer.step().  A gate
    that learns its decay also receives d_q = -a exp(row_loss) / (2n) through q.
    optimizer: any torch.optim over gate.parameters().  -> the mean mixed loss per step (Python floats, before that step's
    update).  The model's parameters and mode are left as found."""
    import model as M
    if not isinstance(gate, CopyGate):
        raise ValueError('fit_gate fits a recurrence.CopyGate')
    gate.check()                                                        # (a non-finite parameter is refused before any launch)
    store = M._observed_store(obs)
    idx = M._observed_positions(store, idx)
    max_batch = max(1, int(max_batch))
    n = len(idx)
    dev = gate.logit.device
    was_training = model.training
    model.eval()
    out = []
    try:
        for _ in range(int(steps)):
            optimizer.zero_grad()
            total = torch.zeros((), device=dev)
            for c in range(0, n, max_batch):
                part = idx[c:c + max_batch]
                sub_pred, ob_pred = model.observed_scores(obs, part)
                rows = CopyRows(store, part, gate)
                m = len(part)
                for k, (pred, gold) in enumerate(((ob_pred, rows_gold(store, part, 'ob')), (sub_pred, rows_gold(store, part, 'sub')))):
                    a, q = rows.a_seq[k * m:(k + 1) * m], rows.q_seq[k * m:(k + 1) * m]
                    row_loss, d_a = K.mix_ce(pred, gold, a.detach().contiguous(), q.detach().contiguous(), 1.0 / (2 * n), False)
                    a.backward(d_a, retain_graph=True)
                    if q.requires_grad:                                  # (a learned decay: dL/dq = -a / m = -a exp(L))
                        import ops
                        q.backward(ops.copy_q_grad(a.detach(), row_loss, 1.0 / (2 * n)), retain_graph=True)
                    total = total + row_loss.sum() / (2 * n)
            optimizer.step()
            out.append(total)
    finally:
        model.train(was_training)
    return [float(x) for x in torch.stack(out).cpu()] if out else []


def rows_gold(store, idx, name):
    """The gold column (int32 device [n]) of side `name` of the stream positions idx: the object for 'ob', the subject for
    'sub'."""
    pos = torch.from_numpy(np.ascontiguousarray(idx, dtype=np.int64)).to(store.device)
    return store.t['q_o' if name == 'ob' else 'q_s'][pos].contiguous()


def _query_store(obs, queries, as_of):
    import model as M
    return M._query_store(obs, queries, as_of)


def evaluate(obs, queries, prior, as_of=None, all_triplets=None, max_batch=4096):
    """The model-free BASELINE under the observed protocol: the labelled queries [n, 4] = (s, r, o, t) ranked by the
    recurrence prior alone -- uniform logits through the mix kernel, then the rank_rows3 tail and the filter lists of
    RENet.evaluate_forecast.  -> ({'raw', 'filtered', 'time_filtered'}, loss[n]) in evaluate_forecast's layout: float64
    ranks [n, 2] = (rank_sub, rank_ob), ties averaged; loss the sum of the two directions' -log p[gold].  as_of: as there
    (None: each query's t).  all_triplets None: the base stream's facts.  A row without history is one N-way tie."""
    _checked(prior)
    qs = _query_store(obs, queries, as_of)
    tr = qs.quads
    s, r, o, t = tr[:, 0], tr[:, 1], tr[:, 2], tr[:, 3]
    if min(s.min(), o.min()) < 0 or max(s.max(), o.max()) >= qs.num_ent:
        raise ValueError('recurrence.evaluate takes labelled queries: both subject and object present')
    dev, n = qs.device, qs.n_quads
    max_batch = max(1, int(max_batch))
    index = FI.filter_index_for(qs, all_triplets if all_triplets is not None else qs.facts)
    lists = np.stack(index.ranges_both_host('s', np.stack((o, r, t), axis=1)) +
                     index.ranges_both_host('o', np.stack((s, r, t), axis=1)) + (s, o)).astype(np.int32)
    up = torch.from_numpy(lists).to(dev)                                # [10, n]: ONE upload for the whole pass
    cols = {side: (index.resident(side, dev), index.resident(side, dev, timed=True)) for side in ('s', 'o')}
    counts = torch.empty(6, n, 2, device=dev, dtype=torch.int32)
    loss = torch.empty(n, 2, device=dev)
    rows = QueryRows(qs, np.arange(n))
    for c in range(0, n, max_batch):
        d = min(n, c + max_batch)
        for col, side, name, lab, base in ((0, 's', 'sub', up[8], 0), (1, 'o', 'ob', up[9], 4)):
            pred = rows.mix(prior, name, None, c, d)
            cnt, ls = K.rank_rows3(pred, lab[c:d], cols[side][0], up[base][c:d], up[base + 1][c:d],
                                   cols[side][1], up[base + 2][c:d], up[base + 3][c:d], want_loss=True)
            counts[:, c:d, col] = cnt
            loss[c:d, col] = ls
    cnt = counts.cpu().numpy().astype(np.float64)
    ranks = {name: cnt[2 * k] + (cnt[2 * k + 1] - 1.0) / 2 + 1 for k, name in enumerate(SETTINGS)}
    return ranks, loss.sum(dim=1).cpu().numpy()


def topk(obs, queries, prior, k=10, all_triplets=None, setting='raw', as_of=None, sides=('sub', 'ob')):
    """The k most probable completions under the recurrence prior alone, in RENet.forecast_topk's layout: {side: (idx,
    score, logp, n_valid)} as device tensors; score = logp = the mixed log-probability.  setting / all_triplets / as_of /
    sides as there; a query whose given side is absent (-1), or without history, has a uniform row (ties by column)."""
    _checked(prior)
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    sides = tuple(sides)
    if not sides or any(name not in SIDES for name in sides):
        raise ValueError("sides must name 'sub', 'ob' or both")
    qs = _query_store(obs, queries, as_of)
    index = FI.filter_index_for(qs, all_triplets if all_triplets is not None else qs.facts) if setting != 'raw' else None
    rows = QueryRows(qs, np.arange(qs.n_quads))
    out = {}
    for name, side, key_col in (('sub', 's', 2), ('ob', 'o', 0)):
        if name not in sides:
            continue
        lists = (None, None, None)
        if index is not None:
            tr = qs.quads
            key, r, t = tr[:, key_col], tr[:, 1], tr[:, 3]
            lists = index.ranges(side, np.stack((key, r, t) if setting == 'time_filtered' else (key, r), axis=1), qs.device)
        out[name] = K.topk_rows(rows.mix(prior, name, None), k, *lists, keep=None)
    return out


def _uniform_events(obs, idx, prior, block_floats):
    """(store, idx, R, N, dev, chunks, blocks) of the model-free event passes: the groups of RENet's event entries (positions
    that share the given entity and the timestamp inside a chunk of gpu_builder.MAX_BOTH positions) and, per sub-block of at
    most block_floats floats, a ZERO block with the offset -log(R * N_ent) through renet_joint_mix_rows."""
    import gpu_builder
    import model as M
    store = M._observed_store(obs)
    idx = M._observed_positions(store, idx)
    R, N, dev = store.num_rels, store.num_ent, store.device
    if R > 1024:
        raise ValueError('event forecasts take at most 1024 relations (renet_joint_row_offsets)')
    mix = EventMix(prior)
    per = max(1, int(block_floats) // max(R * N, 1))
    flat = float(-np.log(float(R) * float(N)))

    def chunks():
        step = gpu_builder.MAX_BOTH
        for c in range(0, len(idx), step):
            ch = M._EventChunk()
            pos = idx[c:c + step]
            ch.c, ch.n = c, len(pos)
            M._event_groups(ch, store, pos, np.arange(2 * len(pos)), mix)
            yield ch

    def blocks(ch, name):
        d = ch.dirs[name]
        for g0 in range(0, len(d.ent), per):
            g1 = min(len(d.ent), g0 + per)
            block = torch.zeros((g1 - g0) * R, N, device=dev)
            off = torch.full(((g1 - g0) * R,), flat, device=dev)
            mix.apply(name, block, off, d.q, g0, g1)
            yield g0, g1, block, off
    return store, idx, R, N, dev, chunks(), blocks


def evaluate_events(obs, idx, prior, all_triplets=None, block_floats=1 << 28):
    """The model-free EVENT baseline under the observed protocol, in RENet.evaluate_events_observed's layout: {'pair':
    {setting: float64 [len, 2]}, 'relation': {setting: float64 [len, 2]}, 'logp': float32 [len, 2]}, column 0 the direction
    sub, column 1 ob.  obs / idx as there (a resident stream or store and its positions; a gpu_builder.QueryStore of labelled
    queries with arange(n) gives stale-history numbers, its as_of cutting the prior).  The same groups, filter lists and tie
    rule; the joint is UNIFORM, J = -log(R * N_ent): zero blocks with that offset go through renet_joint_mix_rows and
    renet_joint_rank_rows.  No encoder, GRU or GEMM launch is made.  A group without history is one R * N_ent-way tie.  To
    be reported with alpha and half_life, beside event numbers of the same protocol only."""
    import model as M
    store, idx, R, N, dev, chunks, blocks = _uniform_events(obs, idx, prior, block_floats)
    with torch.no_grad():
        return M._rank_events(store, idx, R, dev, all_triplets, chunks, blocks)


def topk_events(obs, idx, prior, k=10, all_triplets=None, setting='raw', sides=('sub', 'ob'), block_floats=1 << 28):
    """The k most probable events under the recurrence prior alone, in RENet.predict_events_observed's layout: {'ob': (rel
    int32 [n, k], ent int32 [n, k], logp [n, k], n_valid int32 [n]), 'sub': (...)} as device tensors -- the given entity's
    most frequent (and, with a half-life, most recent) (relation, partner) pairs before as_of, then the unseen pairs, which
    all tie, by relation and entity ascending.  setting / all_triplets / sides as there; it runs predict_events_observed's own
    tail on the mixed uniform blocks of evaluate_events."""
    import model as M
    if setting not in SETTINGS:
        raise ValueError('setting must be one of %s, not %r' % (', '.join(SETTINGS), setting))
    sides = tuple(sides)
    if not sides or any(name not in SIDES for name in sides):
        raise ValueError("sides must name 'sub', 'ob' or both")
    store, idx, R, N, dev, chunks, blocks = _uniform_events(obs, idx, prior, block_floats)
    with torch.no_grad():
        return M._topk_events(store, idx, int(k), R, N, dev, all_triplets, setting, sides, chunks, blocks)
