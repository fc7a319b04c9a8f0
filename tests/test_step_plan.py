"""plan.plan_step against the table recorded at the parent commit (tests/golden/step_plans.json,
made by tools/record_step_plans.py from constructed Trainers): every recorded config selects
exactly the recorded kernel paths, or is rejected with the recorded error.  No GPU."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tools'))

from record_step_plans import dataset_inputs, layout_facts, load_table, plain   # noqa: E402

from cubecobrarecommender_amd.plan import _cdf, plan_step   # noqa: E402
from cubecobrarecommender_amd.trainer import TrainConfig   # noqa: E402

TABLE = load_table(os.path.join(ROOT, 'tests', 'golden', 'step_plans.json'))


def _plan(row):
    ns, rows = dataset_inputs(row)
    return plan_step(TrainConfig(**row['cfg']), cdf=_cdf(ns), data_reg_rows=rows)


def _id(row):
    return ','.join(f'{k}={v}' for k, v in {**row['cfg'], **row['data']}.items())


def test_table_covers_the_grid():
    """Both outcomes are in the table, and it says where it comes from."""
    rows = TABLE['rows']
    assert len(TABLE['recorded_at_commit']) == 40 and not TABLE['package_modified']
    assert sum('error' in r for r in rows) >= 10 and sum('selection' in r for r in rows) >= 400
    for key, values in (('dtype', {'bf16', 'fp32', 'fp8'}), ('d', {64, 128, 256, 512, 1024, 2048}),
                        ('world', {1, 3, 8}), ('reg_mode', {'sampled', 'full'}), ('w1_chunks', {0, 2}),
                        ('wo_tower_frac', {-1.0, 0.0, 1.0})):
        seen = {r['cfg'].get(key, getattr(TrainConfig(V=1), key)) for r in rows}
        assert values <= seen, (key, values - seen)


@pytest.mark.parametrize('row', [r for r in TABLE['rows'] if 'selection' in r], ids=_id)
def test_plan_selects_what_the_parent_selected(row):
    plan = _plan(row)
    got = {key: layout_facts(plan.layout) if key == 'layout' else plain(getattr(plan, key))
           for key in row['selection']}
    assert got == row['selection']


@pytest.mark.parametrize('row', [r for r in TABLE['rows'] if 'error' in r], ids=_id)
def test_plan_rejects_what_the_parent_rejected(row):
    with pytest.raises((ValueError, AssertionError)) as e:
        _plan(row)
    assert {'type': type(e.value).__name__, 'message': str(e.value)} == row['error']
