"""Online learning in the forecast / observe loop (extension of the reference API; the "online" setting RE-GCN, xERTE and
TITer report next to the static one): training steps on the positions of a RESIDENT preprocess.ObservedStream, a step of the
global model on the stream's own per-timestamp distributions, the batched recomputation of the resident global-embedding
table after such a step, and the loop that puts them together.

    RENet.learn_observed(obs, idx, optimizer, ...)          training steps on stream positions (merged two-direction step)
    RENet_global.learn_observed(obs, times, optimizer, ...) one step of the global model (global_model.py)
    ObservedStream.refresh_global(global_model)             a new resident stream with a recomputed `glob` (preprocess.py)
    RENet.evaluate_online(obs, quads, global_model, ...)    forecast t -> observe t -> learn from t, timestamp by timestamp

Numbers of evaluate_online are a FOURTH protocol next to the rollout horizon, the stale-history horizon and the reference's
multi-step state machine: the model that ranks timestamp t has been trained on every evaluated timestamp before t.
"""
import copy

import numpy as np
import torch
from torch.nn.utils.rnn import PackedSequence

import graph as G
import model as M
import ops
import renet_hip as K


# ---- targets of the global model from a stream's own facts -------------------------------------------------------------
def stream_targets(graph_dict, times, num_ent):
    """The CLEAN per-timestamp distributions of the timestamps `times` (any order, repeats allowed) as host CSR arrays:
    {'s': (ptr, col, w), 'o': (ptr, col, w)}, row i the counts of the subjects (objects) among the facts of graph_dict[times[i]]
    divided by the number of facts there -- ptr int64 [n + 1], col int64 ascending per row, w float32.  NOT the bucketing of
    utils.get_true_distribution (utils.py:292-324), which counts the first fact of a timestamp in the previous
    timestamp's row and leaves the last row un-normalised.  KeyError for a timestamp the stream does not hold."""
    out = {}
    times = [int(t) for t in np.asarray(times).reshape(-1)]
    for role, local in (('s', 'ls'), ('o', 'lo')):
        ptr, cols, ws = [0], [], []
        for t in times:
            g = graph_dict[t]
            ids = g.ent[getattr(g, local)]
            if len(ids) and (ids.min() < 0 or ids.max() >= num_ent):
                raise ValueError('entity id outside [0, num_ent)')
            col, cnt = np.unique(ids, return_counts=True)
            cols.append(col.astype(np.int64))
            ws.append((cnt.astype(np.float64) / max(len(ids), 1)).astype(np.float32))
            ptr.append(ptr[-1] + len(col))
        out[role] = (np.asarray(ptr, dtype=np.int64), np.concatenate(cols) if cols else np.zeros(0, np.int64),
                     np.concatenate(ws) if ws else np.zeros(0, np.float32))
    return out


def dense_targets(csr, num_ent):
    """float64 [n, num_ent] of one role of stream_targets (tests, and callers of the dense RENet_global.forward)."""
    ptr, col, w = csr
    out = np.zeros((len(ptr) - 1, num_ent), dtype=np.float64)
    out[np.repeat(np.arange(len(ptr) - 1), np.diff(ptr)), col] = w
    return out


# ---- optimizer steps ---------------------------------------------------------------------------------------------------
def _is_hip_adam(optimizer):
    import parallel
    return isinstance(optimizer, parallel.HipAdam)


def _train_step(module, optimizer, loss_fn, grad_norm, head_passes=1):
    """forward -> backward -> optimizer; -> the loss (device tensor).  parallel.HipAdam: inside its step scope, with its own
    clip, step() and weight registry; any torch.optim.Optimizer: clip_grad_norm_(grad_norm), step(), zero_grad(), as
    train.py:139-142 / pretrain.py:84-87."""
    if _is_hip_adam(optimizer):
        with optimizer.step_scope(head_passes=head_passes):
            loss = loss_fn()
            loss.backward()
            optimizer.step()
        return loss.detach()
    loss = loss_fn()
    loss.backward()
    ops.join_deferred()
    torch.nn.utils.clip_grad_norm_(module.parameters(), grad_norm)
    optimizer.step()
    optimizer.zero_grad()
    K.weights_changed()
    return loss.detach()


# ---- RENet.learn_observed ----------------------------------------------------------------------------------------------
def _learn_observed(self, obs, idx, optimizer, steps=1, batch_size=1024, grad_norm=1.0, prior=None, gate_optimizer=None,
                    event_prior=None):
    """Training steps on the stream positions idx of a resident stream (preprocess.ObservedStream after resident() /
    observe(), or its gpu_builder.ObservedStore): the positions are cut into batches of batch_size <= gpu_builder.MAX_BOTH in
    the given order, and each batch is ONE merged two-direction step in train mode -- prepare_both_device ->
    finish_prepare_device(glob=store.glob), rebuilt when a capacity of the device builder overflowed -> loss_prepared_both ->
    backward -> optimizer -- under the true histories of the stream, with the stream's own global-embedding table.  `steps`
    passes over the batches.  optimizer: a parallel.HipAdam of this model, or any torch.optim.Optimizer over its parameters
    (clip_grad_norm_(grad_norm), step(), zero_grad()).  The model's train / eval mode is restored afterwards.
    -> the batch losses (Python floats, steps * ceil(len(idx) / batch_size) of them; read back once, at the end).
    prior (None: today's path, launch for launch): the entity head's loss goes THROUGH THE COPY MIX of the recurrence prior
    (recurrence.CopyRows of each batch, loss_prepared_both(prep, copy=)), the weights learn what the copy term does not
    explain, and the losses returned are the mixed ones.  A recurrence.RecurrencePrior is a fixed mix; a recurrence.CopyGate
    with a gate_optimizer (any torch.optim over gate.parameters()) learns its gates in the same step -- their gradients stay
    out of the model's clip norm.  A step with a prior is not in the C launch list: it pays the autograd path's host enqueue.
    event_prior (never with prior=): a RecurrencePrior or a CopyGate(per_relation=False) -- every batch gets a
    recurrence.EventCopyRows and the step trains BOTH heads, and with a gate_optimizer the gate, through the JOINT mix
    (loss_prepared_both(prep, event_copy=)): the losses returned are the mean joint losses (relation term at weight 1)."""
    import gpu_builder
    if event_prior is not None:
        import recurrence
        if prior is not None:
            raise ValueError('learn_observed: prior= and event_prior= are two different losses: give one of them')
        recurrence._event_gate(event_prior)
        if gate_optimizer is not None and not isinstance(event_prior, recurrence.CopyGate):
            raise ValueError('learn_observed: gate_optimizer needs event_prior= to be a recurrence.CopyGate')
        if getattr(self, 'gemm_mode', None) == 'bf16s' or K.current_mode() == 'bf16s':
            raise ValueError('learn_observed: event_prior= has no bf16-storage writer: use another GEMM mode')
    elif prior is not None:
        import recurrence
        recurrence._checked(prior)
        if gate_optimizer is not None and not isinstance(prior, recurrence.CopyGate):
            raise ValueError('learn_observed: gate_optimizer needs prior= to be a recurrence.CopyGate')
        if getattr(self, 'gemm_mode', None) == 'bf16s' or K.current_mode() == 'bf16s':
            raise ValueError('learn_observed: prior= has no bf16-storage writer: use another GEMM mode')
        if isinstance(prior, recurrence.CopyGate):
            prior.check()                                               # (a non-finite parameter is refused before any launch)
    elif gate_optimizer is not None:
        raise ValueError('learn_observed: gate_optimizer without prior=')
    store = M._observed_store(obs)
    idx = M._observed_positions(store, idx)
    batch_size, steps = int(batch_size), int(steps)
    if not 1 <= batch_size <= gpu_builder.MAX_BOTH:
        raise ValueError('learn_observed: batch_size must lie in [1, %d]' % gpu_builder.MAX_BOTH)
    if steps < 0:
        raise ValueError('learn_observed: steps must be >= 0')
    was_training = self.training
    losses = []
    self.train()
    try:
        for _ in range(steps):
            for c in range(0, len(idx), batch_size):
                part = idx[c:c + batch_size]
                _, prep = M._observed_prepared(self, store, (part, self.prepare_both_device(part, store)))
                if prep.g.S == 0:
                    raise ValueError('learn_observed: no position of the batch has a history (the first timestamp of a '
                                     'stream): nothing to encode')
                if prior is None and event_prior is None:
                    losses.append(_train_step(self, optimizer, lambda: self.loss_prepared_both(prep), grad_norm))
                    continue
                if gate_optimizer is not None:
                    gate_optimizer.zero_grad()
                if event_prior is not None:
                    rows = recurrence.EventCopyRows(store, part, event_prior)
                    losses.append(_train_step(self, optimizer, lambda: self.loss_prepared_both(prep, event_copy=rows),
                                              grad_norm))
                else:
                    rows = recurrence.CopyRows(store, part, prior)
                    losses.append(_train_step(self, optimizer, lambda: self.loss_prepared_both(prep, copy=rows), grad_norm))
                if gate_optimizer is not None:
                    gate_optimizer.step()
                    gate_optimizer.zero_grad()
    finally:
        self.train(was_training)
    return [float(x) for x in torch.stack(losses).cpu()] if losses else []


# ---- RENet_global.learn_observed ---------------------------------------------------------------------------------------
def _stream_of(obs):
    stream = getattr(obs, 'obs', obs)                                  # (an ObservedStore knows its stream)
    if not hasattr(stream, 'graph_dict') or getattr(stream, 'device', None) is None:
        raise ValueError('the observed stream is not resident: call obs.resident(model, global_model) first')
    return stream


def global_learn_observed(self, obs, times, optimizer, subject=None, grad_norm=1.0):
    """See RENet_global.learn_observed (global_model.py), which binds this."""
    stream = _stream_of(obs)
    dev = self.ent_embeds.device
    t_np = np.asarray(times.cpu() if isinstance(times, torch.Tensor) else times, dtype=np.int64).reshape(-1)
    if len(t_np) == 0:
        raise ValueError('learn_observed: no timestamps')
    t_np = t_np[np.argsort(-t_np, kind='stable')]                      # global_model.py:45: descending
    csr = stream_targets(stream.graph_dict, t_np, self.in_dim)
    # forward()'s pairing: the subject=True head (linear_s) is scored against the OBJECTS' distribution (global_model.py:38-43)
    roles = {True: 'o', False: 's'}
    heads = (True, False) if subject is None else (bool(subject),)
    # ONE upload for the call: the heads' CSR matrices stacked (rows [k n, (k + 1) n) are head k's)
    parts = [csr[roles[h]] for h in heads]
    ptr = parts[0][0]
    for p in parts[1:]:
        ptr = np.concatenate((ptr, p[0][1:] + ptr[-1]))
    targets = ops.SparseTargets(ptr, np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]),
                                self.in_dim, dev)
    n = len(t_np)

    def loss_fn():
        total = None
        for k, h in enumerate(heads):
            linear, reverse = self._head(h)
            packed = self.aggregator(t_np, self.ent_embeds, stream.graph_dict, reverse=reverse)
            _, s_q = self.encoder_global(packed, total_rows=n)
            pred = ops.LinearFn.apply(s_q[0], linear.weight, linear.bias)
            loss = ops.SoftCESparseFn.apply(pred, targets.rows_slice(k * n, (k + 1) * n), 1.0 / n)
            total = loss if total is None else total + loss
        return total

    return float(_train_step(self, optimizer, loss_fn, grad_norm))


# ---- ObservedStream.refresh_global -------------------------------------------------------------------------------------
def global_table_batched(stream, global_model):
    """The table obs.global_table(global_model) as (keys int64 [n], rows [n, H] on the model's device), computed batched
    under no_grad: aggregator.pooled ONCE per timestamp (chunks of <= gpu_builder.MAX_FULL_GRAPHS member graphs from the
    device full-graph builder), then the sliding windows of <= seq_len pooled rows as one packed batch and one
    encoder_global launch per chunk of windows.  Keys and windows are get_global_emb's (global_model.py:57-73): the row of
    timestamp t_k is predict(t_{k+1}) -- the <= seq_len graphs up to and including t_k --, the last one predict(last + time
    unit); a stream that does not start at 0 has the extra key 0 = predict(t_0), taken from predict() itself."""
    import gpu_builder
    gm, agg = global_model, global_model.aggregator
    times = np.asarray(stream.times, dtype=np.int64)
    n, L, H = len(times), int(gm.seq_len), int(gm.h_dim)
    if n < 2:
        raise ValueError('the global-embedding table needs a stream of at least two timestamps (its time unit)')
    graph_dict = stream.graph_dict
    dev = gm.ent_embeds.device
    step = gpu_builder.MAX_FULL_GRAPHS
    with torch.no_grad(), K.gemm_mode(getattr(gm, 'gemm_mode', None)):
        pooled = torch.empty(n, H, device=dev, dtype=torch.float32)
        builder = agg.device_builder
        agg.device_builder = True
        try:
            for c in range(0, n, step):
                pooled[c:c + step] = agg.pooled(times[c:c + step], gm.ent_embeds, graph_dict, False)
        finally:
            agg.device_builder = builder
        rows = torch.empty(n, H, device=dev, dtype=torch.float32)
        for c in range(0, n, step):
            k = np.arange(c, min(c + step, n))
            lens = np.minimum(k + 1, L)
            order = np.argsort(-lens, kind='stable')                   # packed sequences: lengths descending
            lens_s, start_s = lens[order], (k + 1 - lens)[order]
            m, Lc = len(k), int(lens_s[0])
            bs = (lens_s[None, :] > np.arange(Lc)[:, None]).sum(axis=1)
            off = np.concatenate(([0], np.cumsum(bs)))
            seq = np.repeat(np.arange(m), lens_s)
            j = np.arange(len(seq)) - np.repeat(np.cumsum(lens_s) - lens_s, lens_s)
            src = np.empty(len(seq), dtype=np.int64)
            src[off[j] + seq] = start_s[seq] + j                       # packed row (time-major) <- pooled row
            up = G.h2d(np.concatenate((src, c + order)).astype(np.int32), dev)
            x = K.gather_rows(pooled, up[:len(src)])
            _, h = gm.encoder_global(PackedSequence(x, torch.from_numpy(bs.astype(np.int64))), total_rows=m)
            rows[up[len(src):].long()] = h.view(m, H)
        keys = times
        if times[0] != 0:
            first = gm.predict(int(times[0]), graph_dict)[0].detach().reshape(1, H).float()
            keys, rows = np.concatenate(([0], times)), torch.cat((first, rows))
    return keys, rows


def refresh_global(stream, global_model):
    """See ObservedStream.refresh_global (preprocess.py), which binds this."""
    store = stream.device
    if store is None:
        raise ValueError('refresh_global() renews the table of a resident stream: call resident() first')
    keys, rows = global_table_batched(stream, global_model)
    if not np.array_equal(keys, store._glob_times):
        raise ValueError('refresh_global: the resident table does not hold the keys of global_table()')
    new, st = copy.copy(stream), copy.copy(store)
    st.glob = rows
    st._pinned_free = []                                               # (count buffers are owned per store)
    st.obs, new.device = new, st
    return new


# ---- RENet.evaluate_online ---------------------------------------------------------------------------------------------
def _evaluate_online(self, obs, quads, global_model, optimizer, steps=1, replay=0, global_optimizer=None, all_triplets=None,
                     max_batch=4096, batch_size=1024, grad_norm=1.0, prior=None, learn_prior=False, gate_optimizer=None):
    """The forecast / observe / LEARN loop over the labelled, time-sorted quads on the resident stream obs (ending before
    quads[0, 3]).  Per timestamp t of quads, in this order: (1) its facts are ranked with evaluate_forecast on the stream as
    it stands -- nothing of t has been seen, by the stream or by the weights; (2) they are observed (ObservedStream.observe);
    (3) learn_observed runs `steps` steps on their positions followed by those of the `replay` timestamps before t; (4) with a
    global_optimizer, global_model.learn_observed takes one step on t and refresh_global renews the resident table.  Ranking
    runs in eval mode, learning in train mode; the mode found is restored.
    -> (ranks, loss, log): ranks / loss as evaluate_forecast gives them for the whole of quads, in quads order; log one
    {'t', 'losses', 'global_loss'} per timestamp.  self.last_online is the stream after the last timestamp (len(obs) +
    len(quads) facts).  With steps = 0 and no global_optimizer the ranks are those of evaluate_rollout(obs, quads, 1, ...) bit
    for bit.  all_triplets: as there.  These are ONLINE numbers -- a protocol of their own, not comparable with the static
    single-step, stale-horizon, rollout or multi-step ones.
    prior: a recurrence.RecurrencePrior for the forecast half (evaluate_forecast's keyword); the pair tables it reads are
    built at the first timestamp and ride through observe() by the device append.  Learning is not touched by it unless
    learn_prior=True: then prior and gate_optimizer are passed on to learn_observed -- the steps train through the mix, and a
    recurrence.CopyGate with a gate_optimizer learns its gates along the stream (the gate that ranks timestamp t was fitted on
    the timestamps before t: ONLINE numbers WITH A LEARNED GATE, comparable only with numbers of the same protocol)."""
    if (learn_prior and prior is None) or (gate_optimizer is not None and not learn_prior):
        raise ValueError('evaluate_online: learn_prior=True needs prior=, and gate_optimizer needs learn_prior=True')
    store = M._observed_store(obs)
    cur = getattr(store, 'obs', None)
    if cur is None or not hasattr(cur, 'observe'):
        raise ValueError('evaluate_online needs the resident ObservedStream')
    quads = np.asarray(quads.cpu() if isinstance(quads, torch.Tensor) else quads, dtype=np.int64).reshape(-1, 4)
    if len(quads) == 0 or np.any(np.diff(quads[:, 3]) < 0):
        raise ValueError('evaluate_online takes labelled quadruples sorted by time')
    if len(cur.times) and int(cur.times[-1]) >= quads[0, 3]:
        raise ValueError('evaluate_online: the stream must end before the first evaluated timestamp')
    steps, replay = int(steps), int(replay)
    if steps < 0 or replay < 0:
        raise ValueError('evaluate_online: steps and replay must be >= 0')
    known = all_triplets if all_triplets is not None else np.concatenate((cur.allq, quads))
    times, first = np.unique(quads[:, 3], return_index=True)
    ends = list(first[1:]) + [len(quads)]
    ranks, loss, log = {}, [], []
    was_training = self.training
    self.eval()
    try:
        for j, t in enumerate(times):
            q = quads[first[j]:ends[j]]
            r, l = M._evaluate_forecast(self, cur, q, all_triplets=known, max_batch=max_batch, prior=prior)
            for name, v in r.items():
                ranks.setdefault(name, []).append(v)
            loss.append(l)
            index = getattr(cur.device, '_filter_index', None)         # (the index of `known`, handed from store to store)
            n0 = len(cur)
            cur = cur.observe(q, global_model)
            cur.device._filter_index = index
            entry = {'t': int(t), 'losses': [], 'global_loss': None}
            if steps:
                ts = cur.times
                a = int(np.searchsorted(cur.allq[:, 3], ts[max(0, len(ts) - 1 - replay)]))
                pos = np.concatenate((np.arange(n0, len(cur)), np.arange(a, n0)))
                entry['losses'] = _learn_observed(self, cur, pos, optimizer, steps, batch_size, grad_norm,
                                                  prior if learn_prior else None, gate_optimizer if learn_prior else None)
            if global_optimizer is not None:
                entry['global_loss'] = global_model.learn_observed(cur, [int(t)], global_optimizer, grad_norm=grad_norm)
                cur = cur.refresh_global(global_model)
            log.append(entry)
    finally:
        self.train(was_training)
    self.last_online = cur
    return {name: np.concatenate(v) for name, v in ranks.items()}, np.concatenate(loss), log


M.RENet.learn_observed = M._moded(_learn_observed)
M.RENet.evaluate_online = M._moded(_evaluate_online)
