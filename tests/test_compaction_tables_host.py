"""dlsm_compaction_merge_tables, the host form: a compaction's inputs read
straight out of sealed index blocks and data chunks (table_scan.h's rules on the
CPU), against compaction.merge_runs over compaction.table_pairs -- pure Python
that walks each table the way the reference iterator does."""
import numpy as np
import pytest

import dlsm_amd
from dlsm_amd.index_block import build_index_block
from compaction_tables_cases import BAD, CASES, host_args, total, two_files, want


@pytest.mark.parametrize("name", list(CASES))
def test_host_tables_merge_against_the_python_walk_and_merge(name):
    c, w = CASES[name], want(CASES[name])
    caps = dict(zip(("keys_cap", "values_cap", "pair_cap"), w["caps"]))
    got = dlsm_amd.compaction_merge_tables(*host_args(c), c.get("policy", 0), c.get("snapshot", 0), **caps)
    assert list(got[5]) == w["merged"]
    for g, k in zip(got[:5], ("keys", "key_off", "values", "value_off", "src")):
        assert np.array_equal(g, w[k]), k


@pytest.mark.parametrize("name", list(BAD))
def test_host_tables_merge_flags_malformed_tables(name):
    make, flag = BAD[name]
    c = make()
    m = dlsm_amd.compaction_merge_tables(*host_args(c), 1, 100, keys_cap=1 << 12, values_cap=1 << 12, pair_cap=64)[5]
    assert (m[0], m[4]) == (total(c), flag)


def rejected(blocks, files, runs):
    with pytest.raises(dlsm_amd.DlsmError) as e:
        dlsm_amd.compaction_merge_tables(blocks, files, runs, keys_cap=64, values_cap=64, pair_cap=8)
    return e.value.status


def test_host_tables_merge_rejects_bad_arguments():
    blocks, files, _ = host_args(two_files())
    empty = build_index_block([], [])
    big = bytearray(17 * (1 << 23) + 9)  # a header that claims 2^23 entries: only the count is looked at before the rules
    big[-9:-5] = (1 << 23).to_bytes(4, "little")
    for runs, b, f in (([], blocks, files), ([[0]] * 65, blocks, files),         # n_runs outside 1..64
                       ([[0, 2]], blocks, files),                                # a file >= n_files
                       ([[0, 1]], [blocks[0], None], files),                     # no index held
                       ([[0, 1]], blocks, [files[0], None]),                     # no data held
                       ([[0] * 1024], [empty], [None]),                          # more than 1,023 files listed
                       ([[0] * 512], [bytes(big)], [[b"x"]])):                   # more than UINT32_MAX entries
        assert rejected(b, f, runs) == -1, runs[:1]
    assert dlsm_amd.compaction_merge_tables([empty], [None], [[0] * 1023, []], keys_cap=0, values_cap=0, pair_cap=0)[5] == (0,) * 5
