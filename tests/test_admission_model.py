"""The sequential model of the request gate's admission (tests/admission_model.py) against the answers written by hand in
tests/admission_cases.py: every code and every edge the GPU test then holds pm_admit_requests to.  No GPU, no library."""
import pytest

import admission_cases as AC
import admission_model as A


def run_case(c):
    """the model over a case -> (codes per call, model)"""
    m = A.Model()
    for who, (w, n) in c["rate"].items():
        m.set_rate(who, w, n)  # (row = signer: the model keys by whatever it is given)
    got = []
    for now_ms, reqs in c["calls"]:
        batch = []
        for who, gate, age, nonce, beat in reqs:
            flags = (A.FLAG_NO_TIMESTAMP if age is None else 0) | (A.FLAG_NO_NONCE if nonce is None else 0) | (A.FLAG_BEAT if beat else 0)
            ts = 0 if age is None else (now_ms // 1000 - age) & A.U64
            batch.append((gate, who, flags, ts, nonce or b""))
        got.append(m.admit(now_ms, batch))
    return got, m


@pytest.mark.parametrize("name", list(AC.CASES))
def test_the_model_gives_the_answers_written_by_hand(name):
    c = AC.CASES[name]
    got, m = run_case(c)
    assert got == c["want"]
    for who, want in c.get("end_rate", {}).items():
        assert m.rate_of(who) == want, who
    for who, want in c.get("end_beats", {}).items():
        assert m.beat_of(who) == want, who
    if "end_held" in c:
        assert m.counters(c["calls"][-1][0])[1] == c["end_held"]


def test_the_cases_name_every_code():
    seen = {code for c in AC.CASES.values() for call in c["want"] for code in call}
    assert seen == set(range(A.N_CODES))


def test_nonce_format():
    assert A.nonce_ok(b"a" * 16) and A.nonce_ok(b"Z9-" * 21 + b"a") and not A.nonce_ok(b"a" * 15) and not A.nonce_ok(b"a" * 65)
    for c in range(256):
        assert A.nonce_ok(bytes([c]) * 16) == (chr(c).isascii() and (chr(c).isalnum() or c == 0x2D)), c


def test_ttl_edge_millisecond():
    assert A.nonce_live(1000, 1000) and A.nonce_live(61000, 1000) and not A.nonce_live(61001, 1000)
    assert A.nonce_live(999, 1000)  # (the clock stepped back: still there)


def test_the_model_agrees_with_the_header():
    """the codes, flags and the TTL are include/pm_engine.h's"""
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "pm_engine.h")).read()
    for name, val in (("RATE_LIMITED", A.RATE_LIMITED), ("EXPIRED", A.EXPIRED), ("BAD_NONCE", A.BAD_NONCE), ("REPLAY", A.REPLAY),
                      ("NO_NONCE", A.NO_NONCE)):
        assert re.search(r"PM_RQ_%s = %d\b" % (name, val), hdr), name
    assert re.search(r"PM_AD_N_CODES = %d\b" % A.N_CODES, hdr)
    for name, val in (("NO_TIMESTAMP", A.FLAG_NO_TIMESTAMP), ("NO_NONCE", A.FLAG_NO_NONCE), ("BEAT", A.FLAG_BEAT)):
        assert re.search(r"#define PM_RQ_FLAG_%s %du\b" % (name, val), hdr), name
    assert re.search(r"#define PM_RQ_NONCE_TTL_MS %du\b" % A.NONCE_TTL_MS, hdr)
