"""The feature matrix on the host (no GPU): the committed case list covers every pair of levels
that the engine supports, every excluded pair is refused by the engine in its own words, and every
listed case passes fcx_plan_check -- so a combination the engine cannot run is found here, before
any GPU visit (tests/test_gpu_feature_matrix.py runs the same engines)."""
import pytest

import feature_matrix as fm
from fcx import _lib


def test_the_case_list_covers_every_supported_pair():
    pairs = fm.all_pairs()
    excluded = fm.excluded_pairs()
    assert len(pairs) == len(set(pairs)) and excluded <= set(pairs)
    assert len(excluded) == len(fm.EXCLUSIONS)
    assert 10 * len(excluded) <= len(pairs), (len(excluded), len(pairs))  # the table is capped at 10 %
    covered = set()
    for c in fm.CASES:
        levels = {a: getattr(c, a) for a in fm.AXES}
        assert all(levels[a] in fm.AXES[a] for a in fm.AXES), c
        got = fm.pairs_of(levels)
        assert not got & excluded, (fm.describe(c), sorted(got & excluded))
        covered |= got
    missing = set(pairs) - excluded - covered
    assert not missing, sorted(missing)
    assert [c.index for c in fm.CASES] == list(range(len(fm.CASES)))
    print(f"{len(fm.CASES)} cases cover {len(pairs) - len(excluded)} of {len(pairs)} pairs, {len(excluded)} excluded")


def test_the_case_list_is_the_seeded_construction():
    assert fm.build_cases(fm.SEED) == fm.CASES
    assert 20 <= len(fm.CASES) <= 80, len(fm.CASES)


def test_sizes():
    for c in fm.CASES:
        n, sep = fm.sizes(c)
        assert max((n,) + (sep or ())) <= 4400
        assert (n in (129, 300)) == (c.index % 4 == 3)
        assert (sep is None) == (c.grids == "shared")


def plan_check(c):
    """every engine of the case bound and audited on the host; the first refusal is raised
    (a libmem case binds heap arrays here: fcx_host_malloc needs the device, the audit does not
    look at where an array lives)"""
    for v in fm.members(c):
        eng = fm.Member(c, v, True).engine(commit=False)
        try:
            eng.plan_check()
        finally:
            eng.close()


@pytest.mark.parametrize("row", fm.EXCLUSIONS, ids=lambda r: "-".join(l for _, l in r["pair"]))
def test_the_engine_refuses_an_excluded_pair(row):
    c = fm.case_with(row["pair"])
    with pytest.raises(_lib.FcxError) as ex:
        plan_check(c)
    assert ex.value.status == row["status"] and row["text"] in str(ex.value), (row["pair"], ex.value.status, str(ex.value))


@pytest.mark.parametrize("c", fm.CASES, ids=fm.case_id)
def test_the_engine_accepts_every_listed_case(c):
    try:
        plan_check(c)
    except _lib.FcxError as ex:
        pytest.fail(f"{fm.describe(c)}: {ex}")
    # the twins are plain engines of the same cases
    for v in fm.members(c):
        eng = fm.Member(c, v, False).engine(commit=False)
        try:
            eng.plan_check()
        finally:
            eng.close()
