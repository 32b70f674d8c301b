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
preprocess.PairIndex), built on first use and carried through ObservedStream.observe() by renet_pair_append.  Not covered:
rollout (generated facts in a prior are a protocol question of their own), the joint event paths, a relation-free term,
fitting alpha."""
import numpy as np
import torch

import filter_index as FI
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
        return K.recurrence_mix_rows(self.ent[role][c:d], self.rel[c:d], self.t[c:d], self.as_of[c:d], self.tables[role],
                                     t['ent_ptr%d' % role], t['snap_ptr%d' % role], self.base.num_ent, logits, prior.alpha,
                                     prior.inv_half_life, num_cols=self.base.num_ent, want_stats=want_stats)


def _checked(prior):
    if not isinstance(prior, RecurrencePrior):
        raise ValueError('prior must be a recurrence.RecurrencePrior')
    return prior


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
