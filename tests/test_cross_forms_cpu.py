"""Coverage ledger of the cross-feature sweep (tests/cross_forms.py; the GPU half is tests/test_gpu_cross_forms.py): the host layout builder (tilespmv_plan_layout_digest,
no GPU) says which plan forms the seeds and the table reach, and the counts below keep the sweep from going vacuous — a table or generator change that stops reaching the
2-byte form next to split rows, list entries, derived units, partial last tile-rows / tile-columns, shard windows or HYB tiles fails here, not silently on the GPU."""
import numpy as np
import pytest

import cross_forms as X
from tilespmv_amd import api


@pytest.fixture(scope="module")
def ledger():
    return [(c, X.layout_facts(api, c)) for c in map(X.Case, X.SEEDS)]


def test_seed_list_and_matrix_sizes(ledger):
    assert X.SEEDS[:48] == list(range(3000, 3048)) and len(set(X.SEEDS)) == len(X.SEEDS) and sum(map(len, X.GROUPS)) == len(X.SEEDS)
    for c, f in ledger:
        assert c.rowA <= 640 and c.colA <= 960, c
        assert c.hyb == bool(c.seed & 1) and c.nnz == len(c.ci) > 0, c
    for seed in X.HYB_SEEDS:
        f = dict((c.seed, f) for c, f in ledger)[seed]
        assert f["hyb_tiles"] > 0, seed


def test_narrow_requests_get_the_width_their_data_allows(ledger):
    asked_half = [(c, f) for c, f in ledger if c.wants_two_bytes()]
    got = [f["unit_value_bytes"] for _, f in asked_half]
    assert len(asked_half) >= 20 and got.count(2) >= 0.9 * len(got), (len(got), got.count(2))
    asked_float = [(c, f) for c, f in ledger if c.narrow == 2 and c.kind == "float" and not c.value_map]
    assert len(asked_float) >= 5 and all(f["unit_value_bytes"] == 4 for _, f in asked_float), [(c.seed, f["unit_value_bytes"]) for c, f in asked_float]
    assert all(f["unit_value_bytes"] == 4 for c, f in ledger if c.narrow == 1)                                  # value_narrow = 1 on float data
    assert all(f["unit_value_bytes"] == c.dtype().itemsize for c, f in ledger if c.narrow == 0)                 # nobody asked


PROPERTIES = {
    "split tile-rows": lambda c, f: f["num_split_rows"] > 0,
    "list entries": lambda c, f: f["list_entries"] > 0,
    "derived units": lambda c, f: f["derived_units"] > 0,
    "partial last tile-row": lambda c, f: c.rows % 16 != 0,
    "partial last tile-column": lambda c, f: c.cols % 16 != 0,
    "shard window": lambda c, f: c.shard is not None,
    "HYB tiles": lambda c, f: f["hyb_tiles"] > 0,
    "split tile-row that also carries list entries": lambda c, f: f["num_split_rows"] > 0 and f["list_entries"] > 0,
}


@pytest.mark.parametrize("name", sorted(PROPERTIES))
def test_two_byte_plans_meet_every_property_at_least_five_times(ledger, name):
    two = [(c, f) for c, f in ledger if c.wants_two_bytes() and f["unit_value_bytes"] == 2]
    seeds = [c.seed for c, f in two if PROPERTIES[name](c, f)]
    print(name, seeds)
    assert len(seeds) >= 5, (name, seeds)


def test_every_form_builder_and_option_occurs(ledger):
    assert {f["csr_form"] for _, f in ledger} == {1, 2, 3}
    assert {f["entry_mode"] for _, f in ledger} == {0, 1, 2}
    assert {f["desc_bytes"] for _, f in ledger} >= {4, 12}
    assert {f["unit_value_bytes"] for _, f in ledger} == {2, 4, 8}
    for key, want in (("csr_split", {1, 2, 3}), ("entry_mode", {0, 1, 2}), ("desc_dict", {0, 1}), ("dense_mode", {X.DENSE_MFMA, X.DENSE_VALU}), ("absorb", {0, 1}),
                      ("value_narrow", {1, 2}), ("mv_native", {1, 2}), ("strip_cost", {64}), ("split_above", {150})):
        assert {c.opts[key] for c, _ in ledger if key in c.opts} == want, key
    for c, _ in ledger:                                                               # the narrow values only beside the eligible forms
        assert not c.narrow or (c.opts["csr_split"] == 1 and c.opts["entry_mode"] in (0, 2)), c
    for what in ("transpose", "value_map", "device_build", "hyb"):
        assert {bool(getattr(c, what)) for c, _ in ledger} == {False, True}, what
    assert {c.nvec for c, _ in ledger} == {1, 2, 4, 8} and {c.kind for c, _ in ledger} == {"half", "float", "f32"}
    assert {(c.nvec, c.opts["mv_native"]) for c, _ in ledger if c.nvec > 1} == {(n, m) for n in (2, 4, 8) for m in (1, 2)}
    assert {c.rowA % 16 for c, _ in ledger} >= {0, 15, 11, 1}                          # rows_off 0 / 1 / 5 / 15
    # a sharded case really is one: the plan holds the window's rows only
    for c, f in ledger:
        if c.shard:
            assert f["rows"] == min(c.rows, 16 * c.shard[1]) - 16 * c.shard[0] < c.rows, c
