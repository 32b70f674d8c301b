"""CPU tests of preprocess.ObservedStream (the whole dataset as one observed stream: the single-step / ground-truth history
evaluation protocol): its histories and graphs against the oracle's streaming restatement of get_history_graph.py run over
the concatenated stream, the split ranges, a stream without a valid split, the history_len cut -- and that the pass is
attached to the model."""
import numpy as np
import pytest

from helpers import O, fixtures

import observed_stream as S


@pytest.fixture(scope='module')
def splits():
    tr, va, te = S.make()
    S.check_cases(tr, va, te)
    return tr, va, te


def _same_graphs(mine, ref):
    assert list(mine.keys()) == list(ref.keys())
    for t in ref:
        g, og = mine[t], ref[t]
        assert np.array_equal(g.ent, og.ent), t
        src, dst, type_s = g.edges(reverse=False)
        _, _, type_o = g.edges(reverse=True)
        assert np.array_equal(src, og.src) and np.array_equal(dst, og.dst), t
        assert np.array_equal(type_s, og.type_s) and np.array_equal(type_o, og.type_o), t


@pytest.mark.parametrize('history_len', [S.SEQ_LEN, 10])
def test_histories_of_every_split_position_equal_the_oracle_over_the_whole_stream(splits, history_len):
    import preprocess as P
    obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, history_len)
    allq = np.concatenate(splits)
    assert np.array_equal(obs.allq, allq) and len(obs) == len(allq)
    sh, oh, _ = O.build_histories(allq, S.NUM_ENT, history_len=history_len)
    for name in ('train', 'valid', 'test'):
        pos = obs.positions(name)
        assert fixtures.histories_equal(obs.hist_s.to_lists(pos), ([sh[0][i] for i in pos], [sh[1][i] for i in pos])), name
        assert fixtures.histories_equal(obs.hist_o.to_lists(pos), ([oh[0][i] for i in pos], [oh[1][i] for i in pos])), name
    # the cut: no history is longer than history_len, and with the short one some would be
    longest = max(len(h) for h in sh[1])
    assert longest == history_len
    assert int(obs.hist_s.count.max()) == history_len and int(obs.hist_o.count.max()) == history_len
    # a test query sees its own split: the newest step of a late history lies in the test period
    late = obs.positions('test')[-1]
    assert max(obs.hist_s.to_lists([late])[1][0] + obs.hist_o.to_lists([late])[1][0]) >= S.SPLIT_T[1]


def test_graphs_cover_every_timestamp_and_equal_the_oracle(splits):
    import preprocess as P
    obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    _same_graphs(obs.graph_dict, O.build_graph_dict(np.concatenate(splits), S.NUM_RELS))
    assert list(obs.graph_dict.keys()) == list(range(S.NUM_T)) and obs.times.tolist() == list(range(S.NUM_T))


def test_split_ranges(splits):
    import preprocess as P
    tr, va, te = splits
    obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    assert obs.ranges == {'train': (0, len(tr)), 'valid': (len(tr), len(tr) + len(va)),
                          'test': (len(tr) + len(va), len(tr) + len(va) + len(te))}
    for name, q in zip(('train', 'valid', 'test'), splits):
        assert np.array_equal(obs.allq[obs.positions(name)], q)
    assert obs.device is None                                   # host arrays only until resident()


@pytest.mark.parametrize('form', ['pair', 'none'])
def test_stream_without_a_valid_split(splits, form):
    import preprocess as P
    tr, va, te = splits
    train = np.concatenate((tr, va))
    obs = P.ObservedStream((train, te) if form == 'pair' else (train, None, te), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    assert sorted(obs.ranges) == ['test', 'train'] and obs.ranges['test'] == (len(train), len(train) + len(te))
    whole = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    pos = obs.positions('test')
    assert fixtures.histories_equal(obs.hist_s.to_lists(pos), whole.hist_s.to_lists(whole.positions('test')))
    with pytest.raises(KeyError):
        obs.positions('valid')
    with pytest.raises(ValueError):
        P.ObservedStream((tr,), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    with pytest.raises(ValueError):
        P.ObservedStream((te, tr), S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)        # not in time order


def test_the_pass_is_attached_to_the_model_and_wants_a_resident_stream(splits):
    import model as M
    import preprocess as P
    for name in ('observed_scores', 'evaluate_observed', 'predict_topk_observed'):
        assert callable(getattr(M.RENet, name))
    net = M.RENet(S.NUM_ENT, 100, S.NUM_RELS, seq_len=S.SEQ_LEN)
    obs = P.ObservedStream(splits, S.NUM_ENT, S.NUM_RELS, S.SEQ_LEN)
    with pytest.raises(ValueError, match='resident'):
        net.evaluate_observed(obs, obs.positions('test'))
    import inspect
    assert 'glob' in inspect.signature(M.RENet.finish_prepare_device).parameters

