"""The index-stream reference at the GPU test's case list: oracle.pcg64.PCG64State against numpy itself, and the
list's coverage of the Lemire rejection branch (a condition on the inputs, not on the kernel)."""

import numpy as np

import index_stream_cases as IC


def test_reference_matches_numpy_at_the_case_list():
    for seed, high, n in IC.all_cases():
        r = np.random.default_rng(seed)
        for before, idx, after, _ in IC.reference(seed, high, n):
            st = r.bit_generator.state
            assert before == [st["state"]["state"] >> 64, st["state"]["state"] & (2**64 - 1), st["state"]["inc"] >> 64,
                              st["state"]["inc"] & (2**64 - 1), st["has_uint32"], st["uinteger"]]
            np.testing.assert_array_equal(idx, r.integers(0, high, size=n))
            st = r.bit_generator.state
            assert after[4:] == [st["has_uint32"], st["uinteger"]] and (after[0] << 64) | after[1] == st["state"]["state"]


def test_case_list_reaches_the_rejection_branch():
    calls = [(c, k, ev) for c in IC.all_cases() for k, (before, _, _, ev) in enumerate(IC.reference(*c))]
    entered = [before[4] for c in IC.all_cases() for before, _, _, _ in IC.reference(*c)]
    assert 0 in entered and 1 in entered
    assert any(ev["buffered_rejected"] for _, _, ev in calls), "no call whose buffered half-word is rejected"
    assert any(ev["last"] == "lo" for _, _, ev in calls) and any(ev["last"] == "hi" for _, _, ev in calls)
    assert any(ev["last"] == "buf" for _, _, ev in calls)  # n = 1 served from the buffered half alone
    assert any(ev["rounds"] >= 3 for _, _, ev in calls)
    assert sum(ev["rejections"] for _, _, ev in calls) >= 100
    # the last accepted candidate is not always the last candidate of its round, and a rejected lane precedes
    # accepted ones: both follow from rejections inside multi-draw calls
    assert any(ev["rejections"] > 0 and c[2] >= 63 for c, _, ev in calls)
