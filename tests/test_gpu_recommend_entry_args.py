"""The argument checks of the six batched recommend entries (csrc/recbatch.hip), called directly:
every refused call returns CC_ERR_ARG with the entry's own message, the first violated rule's when
two are violated, and launches nothing; R == 0 returns 0 and launches nothing.  The messages are
the ABI's, byte for byte, written out per entry.  No call here reaches a kernel."""
import numpy as np
import pytest
import torch

from cubecobrarecommender_amd import _lib as L
from cubecobrarecommender_amd.recommender import pack_cubes
from tests.test_gpu_recommend_batch import mixed_batch, model_of

pytestmark = pytest.mark.gpu

CC_ERR_ARG = -1
SHAPES = [(63, 64), (1001, 128)]
AMOUNT = 40

# entry -> rule -> cc_last_error_string() of a call that violates it
MESSAGES = {
    'cc_recommend_batch_fp32': {
        'null': 'cc_recommend_batch_fp32: null pointer',
        'max_n': 'cc_recommend_batch_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_fp32: d must be a multiple of 64 in [64, 1024]',
        'amount': 'cc_recommend_batch_fp32: amount above cc_recommend_batch_max_amount()',
        'ws': 'cc_recommend_batch_fp32: ws must be 256-byte aligned',
    },
    'cc_recommend_batch_pool_fp32': {
        'null': 'cc_recommend_batch_pool_fp32: null pointer',
        'pool_of_row': 'cc_recommend_batch_pool_fp32: null pointer',
        'n_pools': 'cc_recommend_batch_pool_fp32: n_pools is negative',
        'pools': 'cc_recommend_batch_pool_fp32: pools is null with n_pools > 0',
        'max_n': 'cc_recommend_batch_pool_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_pool_fp32: d must be a multiple of 64 in [64, 1024]',
        'amount': 'cc_recommend_batch_pool_fp32: amount above cc_recommend_batch_max_amount()',
        'ws': 'cc_recommend_batch_pool_fp32: ws must be 256-byte aligned',
    },
    'cc_recommend_batch_rank_fp32': {
        'null': 'cc_recommend_batch_rank_fp32: null pointer',
        'max_n': 'cc_recommend_batch_rank_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_rank_fp32: d must be a multiple of 64 in [64, 1024]',
        'ws': 'cc_recommend_batch_rank_fp32: ws must be 256-byte aligned',
    },
    'cc_recommend_batch_rank_pool_fp32': {
        'null': 'cc_recommend_batch_rank_pool_fp32: null pointer',
        'pool_of_row': 'cc_recommend_batch_rank_pool_fp32: null pointer',
        'n_pools': 'cc_recommend_batch_rank_pool_fp32: n_pools is negative',
        'pools': 'cc_recommend_batch_rank_pool_fp32: pools is null with n_pools > 0',
        'max_n': 'cc_recommend_batch_rank_pool_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_rank_pool_fp32: d must be a multiple of 64 in [64, 1024]',
        'ws': 'cc_recommend_batch_rank_pool_fp32: ws must be 256-byte aligned',
    },
    'cc_recommend_batch_target_ranks_fp32': {
        'null': 'cc_recommend_batch_target_ranks_fp32: null pointer',
        'max_n': 'cc_recommend_batch_target_ranks_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_target_ranks_fp32: d must be a multiple of 64 in [64, 1024]',
        'n_cutoffs': 'cc_recommend_batch_target_ranks_fp32: n_cutoffs outside 0..8, or cutoffs null',
        'ws': 'cc_recommend_batch_target_ranks_fp32: ws must be 256-byte aligned',
    },
    'cc_recommend_batch_target_ranks_pool_fp32': {
        'null': 'cc_recommend_batch_target_ranks_pool_fp32: null pointer',
        'pool_of_row': 'cc_recommend_batch_target_ranks_pool_fp32: null pointer',
        'n_pools': 'cc_recommend_batch_target_ranks_pool_fp32: n_pools is negative',
        'pools': 'cc_recommend_batch_target_ranks_pool_fp32: pools is null with n_pools > 0',
        'max_n': 'cc_recommend_batch_target_ranks_pool_fp32: V/R/max_n',
        'd': 'cc_recommend_batch_target_ranks_pool_fp32: d must be a multiple of 64 in [64, 1024]',
        'n_cutoffs': 'cc_recommend_batch_target_ranks_pool_fp32: n_cutoffs outside 0..8, or cutoffs null',
        'ws': 'cc_recommend_batch_target_ranks_pool_fp32: ws must be 256-byte aligned',
    },
}
# the order of an entry's checks: of two violated rules the earlier one is reported
ORDER = ['null', 'pool_of_row', 'n_pools', 'pools', 'max_n', 'd', 'amount', 'n_cutoffs', 'ws']
REQUIRED = {   # the pointers behind an entry's own "null pointer" (probs, hits and cutoffs may be null)
    'add': ['params', 'row_ptr', 'idx', 'ws', 'n_add', 'additions', 'add_vals', 'cut_vals'],
    'tgt': ['params', 'row_ptr', 'idx', 'tgt_ptr', 'tgt', 'ws', 'ranks', 'tgt_vals', 'cut_vals'],
}


class Call:
    """One entry's valid argument list on 11 rows, every output and the workspace holding junk."""

    def __init__(self, entry, V, d):
        _, rec = model_of(V, d)
        cubes = mixed_batch(V)
        self.entry, self.V, self.kind = entry, V, 'tgt' if 'target_ranks' in entry else 'add'
        dev, R = rec.dev, len(cubes)
        row_ptr, idx, max_n, _, _ = pack_cubes(cubes, V)
        ws_bytes = int(getattr(L.lib(), entry.replace('_fp32', '_ws_size'))(V, d, R, max_n))
        self.ws = torch.full((ws_bytes // 4 + 64,), -1, device=dev, dtype=torch.int32)
        assert self.ws.data_ptr() % 256 == 0

        def ints(n, fill=77):
            return torch.full((max(n, 1),), fill, device=dev, dtype=torch.int32)

        def flts(n):
            return torch.full((max(n, 1),), 7.0, device=dev)
        self.inputs = [torch.from_numpy(row_ptr).to(dev), torch.from_numpy(idx).to(dev)]
        a = {'params': L.ptr(rec.params), 'V': V, 'd': d, 'R': R, 'row_ptr': L.ptr(self.inputs[0]),
             'idx': L.ptr(self.inputs[1]), 'max_n': max_n}
        if self.kind == 'add':
            self.outs = {'n_add': ints(R), 'additions': ints(R * AMOUNT), 'add_vals': flts(R * AMOUNT)}
            a.update(amount=AMOUNT, ws=L.ptr(self.ws), **{k: L.ptr(t) for k, t in self.outs.items()})
        else:
            tgt_ptr = np.arange(R + 1, dtype=np.int32)              # one target a row: card 0
            self.inputs += [torch.from_numpy(tgt_ptr).to(dev), ints(R, 0), ints(8, 5)]
            self.outs = {'ranks': ints(R), 'tgt_vals': flts(R),
                         'hits': torch.full((10,), 77, device=dev, dtype=torch.int64)}
            a.update(tgt_ptr=L.ptr(self.inputs[2]), tgt=L.ptr(self.inputs[3]), cutoffs=L.ptr(self.inputs[4]),
                     n_cutoffs=2, ws=L.ptr(self.ws), **{k: L.ptr(t) for k, t in self.outs.items()})
        self.outs.update(cut_vals=flts(len(idx)), probs=flts(R * V))
        a.update(cut_vals=L.ptr(self.outs['cut_vals']), probs=L.ptr(self.outs['probs']))
        if '_pool_' in entry:
            self.inputs += [torch.full((2, (V + 31) // 32), -1, device=dev, dtype=torch.int32), ints(R, 1)]
            a.update(pools=L.ptr(self.inputs[-2]), n_pools=2, pool_of_row=L.ptr(self.inputs[-1]))
        a['stream'] = L.stream_ptr()
        self.args = a
        self.junk = {k: t.clone() for k, t in self.outs.items()}
        torch.cuda.synchronize()

    def fault(self, rule):
        """The arguments that violate `rule` (and no other)."""
        if rule == 'ws':
            return {'ws': L.C.c_void_p(self.ws.data_ptr() + 4)}
        return {'null': {'cut_vals': None}, 'pool_of_row': {'pool_of_row': None}, 'n_pools': {'n_pools': -1},
                'pools': {'pools': None}, 'max_n': {'max_n': self.V + 1}, 'd': {'d': 96},
                'amount': {'amount': int(L.lib().cc_recommend_batch_max_amount()) + 1},
                'n_cutoffs': {'n_cutoffs': 9}}[rule]

    def run(self, **over):
        """(rc, message) of the call with `over` in place of the valid arguments; the outputs and the
        workspace are as they were, so nothing was launched."""
        rc = getattr(L.lib(), self.entry)(*{**self.args, **over}.values())
        msg = L.lib().cc_last_error_string().decode()
        torch.cuda.synchronize()
        for k, t in self.outs.items():
            assert torch.equal(t, self.junk[k]), (self.entry, over, k)
        assert bool((self.ws == -1).all()), (self.entry, over)
        return rc, msg


_calls = {}


def call_of(entry, V, d):
    if (entry, V, d) not in _calls:
        _calls[(entry, V, d)] = Call(entry, V, d)
    return _calls[(entry, V, d)]


@pytest.mark.parametrize('V,d', SHAPES)
@pytest.mark.parametrize('entry', list(MESSAGES))
def test_each_rule(entry, V, d):
    c = call_of(entry, V, d)
    for rule, want in MESSAGES[entry].items():
        assert c.run(**c.fault(rule)) == (CC_ERR_ARG, want), rule
    for name in REQUIRED[c.kind]:                                   # every required pointer
        assert c.run(**{name: None}) == (CC_ERR_ARG, MESSAGES[entry]['null']), name


@pytest.mark.parametrize('V,d', SHAPES)
@pytest.mark.parametrize('entry', list(MESSAGES))
def test_two_rules_report_the_first(entry, V, d):
    c = call_of(entry, V, d)
    rules = [r for r in ORDER if r in MESSAGES[entry]]
    assert len(rules) == len(MESSAGES[entry])
    for i, first in enumerate(rules):
        for second in rules[i + 1:]:
            assert c.run(**c.fault(first), **c.fault(second)) == (CC_ERR_ARG, MESSAGES[entry][first]), (first, second)


@pytest.mark.parametrize('V,d', SHAPES)
@pytest.mark.parametrize('entry', list(MESSAGES))
def test_no_rows(entry, V, d):
    c = call_of(entry, V, d)
    assert c.run(R=0)[0] == 0
    assert c.run(R=0, **c.fault('ws')) == (CC_ERR_ARG, MESSAGES[entry]['ws'])     # checked before R == 0
