"""_lib.SIGNATURES derives the twelve batched recommend signatures (six entries, six _ws_size) from
shared pieces; here they are spelled out item by item, as include/ccrec.h declares them."""
import ctypes as C

from cubecobrarecommender_amd import _lib as L

_P, _I32, _SZ = C.c_void_p, C.c_int32, C.c_size_t

SPELLED_OUT = {
    'cc_recommend_batch_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P, _P]),
    'cc_recommend_batch_rank_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_rank_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P,
                                               _P]),
    'cc_recommend_batch_target_ranks_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_target_ranks_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _P, _I32, _P,
                                                       _P, _P, _P, _P, _P, _P]),
    'cc_recommend_batch_pool_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_pool_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P, _P,
                                               _P, _I32, _P, _P]),
    'cc_recommend_batch_rank_pool_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_rank_pool_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _I32, _P, _P, _P, _P, _P,
                                                    _P, _P, _I32, _P, _P]),
    'cc_recommend_batch_target_ranks_pool_ws_size': (_SZ, [_I32, _I32, _I32, _I32]),
    'cc_recommend_batch_target_ranks_pool_fp32': (C.c_int, [_P, _I32, _I32, _I32, _P, _P, _I32, _P, _P, _P, _I32,
                                                            _P, _P, _P, _P, _P, _P, _P, _I32, _P, _P]),
}


def test_the_derived_signatures_are_the_spelled_out_ones():
    derived = {k: v for k, v in L.SIGNATURES.items()
               if k.startswith('cc_recommend_batch') and k not in ('cc_recommend_batch_max_amount',
                                                                   'cc_recommend_batch_loss_ws_size',
                                                                   'cc_recommend_batch_loss_fp32')}
    assert set(derived) == set(SPELLED_OUT)
    for name, (res, args) in SPELLED_OUT.items():
        assert derived[name][0] is res, name
        assert len(derived[name][1]) == len(args) and all(a is b for a, b in zip(derived[name][1], args)), name
