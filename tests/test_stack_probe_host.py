"""The decisions of the stack-buffer probe (EnvSet.pickStackBuffer) on made-up timings: no device, no library load.

Every expected value below is worked out by hand from the probe's rules:
  * candidate k comes from kinds[0] for k = 0, from the rest of ``kinds`` cyclically otherwise;
  * room = candidates that half of the free memory holds, fit = min(asked, room) but at least 1;
  * the search is extended once, by min(n, room - n) candidates, when no candidates were handed in (``among``),
    3 <= n < room, min(medians) > 0.93 * medians[0] and medians[0] >= 0.1 ms;
  * chosen = argmin(median); the "uniform" note needs more than two candidates and min(medians) > 0.9 * medians[0];
  * the share check applies to d >= 7 stacks that are not u8; with a process-wide bias > 0 the bias is kept iff the
    biased write is not slower than the write with equal shares.
"""
import torch

from toric_rl_decoder_amd import stackbuf as S

GB = 10 ** 9
REPORT_KEYS = {"candidates", "candidates_asked", "candidates_added_because_uniform", "write_ms", "write_ms_min", "chosen",
               "probe_ms_chosen", "writes_per_candidate", "kinds", "addresses"}


def test_kind_of_candidate_k():
    kinds = lambda names, n: [S.candidate_kind(names, k) for k in range(n)]
    assert kinds(("torch", "chunked"), 4) == ["torch", "chunked", "chunked", "chunked"]
    assert kinds(("torch", "a", "b"), 5) == ["torch", "a", "b", "a", "b"]
    assert kinds(("chunked",), 3) == ["chunked", "chunked", "chunked"]


def test_room_and_fit():
    assert S.candidates_that_fit(100 * GB, 5 * GB, 24) == (10, 10)      # half of 100 GB holds ten of 5 GB
    assert S.candidates_that_fit(100 * GB, 5 * GB, 4) == (10, 4)
    assert S.candidates_that_fit(100 * GB, 60 * GB, 4) == (0, 1)        # larger than half: one is tried all the same
    assert S.candidates_that_fit(100 * GB, 5 * GB, 0) == (10, 1)        # asked < 1 counts as 1


def test_extension_rule():
    near = [0.36, 0.35, 0.37]                                           # 0.35 > 0.93 * 0.36 = 0.3348: nobody stands out
    assert S.candidates_to_add(near, 10, False) == 3                    # as many again
    assert S.candidates_to_add(near, 4, False) == 1                     # ... but never more than room
    assert S.candidates_to_add(near, 3, False) == 0                     # no room left
    assert S.candidates_to_add([0.36, 0.30, 0.37], 10, False) == 0      # 0.30 <= 0.3348: candidate 1 stands out
    assert S.candidates_to_add([0.05, 0.05, 0.05], 10, False) == 0      # under 0.1 ms: not about bandwidth
    assert S.candidates_to_add([0.36, 0.35], 10, False) == 0            # two candidates
    assert S.candidates_to_add(near, 10, True) == 0                     # a re-probe of given buffers (among)


def test_median_decides_and_ties_go_to_the_lower_index():
    steady, outlier = [0.36, 0.36, 0.36, 0.36], [0.10, 0.40, 0.40, 0.40]
    ms, ms_min, chosen = S.verdict([steady, outlier])
    assert ms == [0.36, 0.40] and ms_min == [0.36, 0.10] and chosen == 0
    assert S.verdict([outlier, steady])[2] == 1
    assert S.verdict([[0.3, 0.3, 0.3], [0.3, 0.3, 0.3], [0.31, 0.31, 0.31]])[2] == 0


def _report(medians, **kw):
    samples = [[m, m, m] for m in medians]
    n = len(medians)
    return S.probe_report(samples, kw.pop("asked", n), kw.pop("added", 0), [S.TORCH_EMPTY] + [S.CHUNKED] * (n - 1),
                          [hex(0x1000 * (i + 1)) for i in range(n)], **kw)


def test_uniform_note():
    assert "uniform" in _report([0.36, 0.35, 0.37])                     # 0.35 > 0.9 * 0.36 = 0.324
    assert "uniform" not in _report([0.36, 0.30])                       # two candidates
    assert "uniform" not in _report([0.36, 0.30, 0.37])                 # 0.30 <= 0.324
    assert "profiles/r03_stack_write_ab.txt" in _report([0.36, 0.35, 0.37])["uniform"]


def test_share_check():
    assert S.share_check_applies(7, torch.float32) and S.share_check_applies(9, torch.bfloat16)
    assert not S.share_check_applies(5, torch.float32) and not S.share_check_applies(7, torch.uint8)
    assert S.shares_outcome(0) == {"bias": 0}                           # process-wide bias 0: nothing to compare
    assert S.shares_outcome(2, 0.30, 0.30) == {"bias": 2, "write_ms_biased": 0.30, "write_ms_equal_shares": 0.30}
    assert S.shares_outcome(2, 0.29, 0.30)["bias"] == 2
    assert S.shares_outcome(2, 0.31, 0.30) == {"bias": 0, "write_ms_biased": 0.31, "write_ms_equal_shares": 0.30}


def test_report():
    rep = _report([0.36, 0.30, 0.37], asked=3)                          # no share check (d = 5, or a u8 stack)
    assert set(rep) == REPORT_KEYS
    assert rep["candidates"] == rep["candidates_asked"] == 3 and rep["candidates_added_because_uniform"] == 0
    assert rep["write_ms"] == rep["write_ms_min"] == [0.36, 0.30, 0.37] and rep["chosen"] == 1
    assert rep["probe_ms_chosen"] == 0.30 and rep["writes_per_candidate"] == 3
    assert rep["kinds"] == ["torch.empty", "alloc_stack (2 MiB chunks)", "alloc_stack (2 MiB chunks)"]
    assert rep["addresses"] == ["0x1000", "0x2000", "0x3000"]
    assert S.REPROBED == "re-probed"

    rep = _report([0.36, 0.30, 0.37], shares=S.shares_outcome(0))
    assert set(rep) == REPORT_KEYS | {"xcd_bias"} and rep["xcd_bias"] == {"bias": 0} and rep["probe_ms_chosen"] == 0.30

    rep = _report([0.36, 0.30, 0.37], shares=S.shares_outcome(2, 0.29, 0.31))
    assert set(rep) == REPORT_KEYS | {"xcd_bias"} and set(rep["xcd_bias"]) == {"bias", "write_ms_biased", "write_ms_equal_shares"}
    assert rep["probe_ms_chosen"] == 0.29                               # min(biased, equal shares), not the median above
    assert _report([0.36, 0.30, 0.37], shares=S.shares_outcome(2, 0.31, 0.28))["probe_ms_chosen"] == 0.28

    rep = _report([0.36, 0.35, 0.37, 0.36, 0.35, 0.34], asked=3, added=3)
    assert set(rep) == REPORT_KEYS | {"uniform"}
    assert rep["candidates"] == 6 and rep["candidates_asked"] == 3 and rep["candidates_added_because_uniform"] == 3 and rep["chosen"] == 5
