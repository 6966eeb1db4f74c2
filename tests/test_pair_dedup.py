"""Duplicate QPs in the two-QPs-per-wave kernel (csrc/mpc_pair.hpp): per aligned group of 16
instances, an instance whose contact word, x0, xref and lin equal -- bit for bit -- those of the
group's first instance with that word (its leader) is covered: not solved, its rows written by
the leader's wavefront.  Equality of outputs cannot tell "covered" from "solved to the same
bits", so every test reads the kernel's covered-instance counter (mpcqp_count_covered) and
compares it with the count recomputed here from the inputs' bit patterns.  MPCQP_PAIR_DEDUP=0 at
context creation turns the coverage off (every instance solves itself): the same binary gives
the reference run.  Outputs are pre-filled with sentinels, so a row nobody wrote shows.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL_U = 1e-8
PAIR_NF = 30  # free variables a half of the paired kernel holds; more: the overflow kernel


def u_close(U, U0):
    return np.abs(np.asarray(U) - U0).max() <= TOL_U * max(1.0, np.abs(U0).max())


def covered_mask(batch, N):
    """which instances the kernel covers, from the bit patterns: leader = lowest index of the
    aligned group of 16 with the same contact word; covered = leader is another instance and
    x0 / xref / lin equal the leader's as 64-bit integers.  An instance that may exceed the
    paired kernel's capacity (three free forces per foot in contact) goes to the overflow
    kernel and is never covered."""
    ct = np.ascontiguousarray(batch["contact"]).astype(np.uint64)
    B = ct.shape[0]
    rows = np.concatenate([np.ascontiguousarray(batch[k], dtype=np.float64).reshape(B, -1)
                           for k in ("x0", "xref", "lin")], axis=1).view(np.uint64)
    sched = (1 << (2 * N)) - 1
    out = np.zeros(B, dtype=bool)
    for g0 in range(0, B, 16):
        for i in range(g0, min(g0 + 16, B)):
            lead = next(j for j in range(g0, i + 1) if ct[j] == ct[i])
            fits = 3 * bin(int(ct[i]) & sched).count("1") <= PAIR_NF
            out[i] = lead != i and fits and np.array_equal(rows[i], rows[lead])
    return out


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def run(p, batch, monkeypatch, dedup, w4=False):
    """one solve on sentinel-filled outputs -> outputs, covered count, the context's crash caps"""
    import torch
    from mpcqp.engine import BatchEngine
    if dedup:
        monkeypatch.delenv("MPCQP_PAIR_DEDUP", raising=False)
    else:
        monkeypatch.setenv("MPCQP_PAIR_DEDUP", "0")
    if w4:
        monkeypatch.setenv("MPCQP_PAIR_W4_MIN", "1")
    else:
        monkeypatch.delenv("MPCQP_PAIR_W4_MIN", raising=False)
    eng = BatchEngine(p)
    assert eng.fused_kernel == "k_mpc_pair" and eng.pair_dedup == dedup
    B = batch["contact"].shape[0]
    # the build the launch takes: the 4-wave one from pair_w4_min instances per launch
    assert (0 < eng.pair_w4_min <= B) == w4, (eng.pair_w4_min, B)
    d = eng.upload(batch)
    d["U"].fill_(float("nan"))
    d["cost"].fill_(float("nan"))
    d["status"].fill_(99)
    d["iters"].fill_(-1)
    torch.cuda.synchronize()
    eng.count_covered(True)
    eng.solve(d)
    eng.sync()
    cov, launches = eng.covered()
    eng.count_covered(False)
    assert launches == 1
    o = {k: d[k].cpu().numpy() for k in ("U", "cost", "status", "iters")}
    o["covered"] = cov
    o["crash"] = eng.crash
    eng.close()
    assert not np.isnan(o["U"]).any() and not np.isnan(o["cost"]).any()  # no sentinel left
    assert (o["status"] != 99).all() and (o["iters"] >= 0).all()
    return o


def assert_same_bits(a, b):
    for k in ("U", "cost", "status", "iters"):
        np.testing.assert_array_equal(bits(a[k]), bits(b[k]), err_msg=k)


def assert_oracle(orc, p, batch, o, idx=None):
    q = dict(p)
    q["crash"] = tuple(o["crash"])
    sel = slice(None) if idx is None else idx
    ref = orc.srbm_batch(q, batch["x0"][sel], batch["xref"][sel], batch["lin"][sel],
                         batch["contact"][sel])
    np.testing.assert_array_equal(o["status"][sel], ref["status"])
    Uo = o["U"][sel]
    bad = [j for j in range(Uo.shape[0]) if not u_close(Uo[j], ref["U"][j])]
    assert not bad, bad[:10]
    np.testing.assert_allclose(o["cost"][sel], ref["cost"], rtol=1e-9, atol=1e-9)


@pytest.mark.parametrize("w4", [False, True])
def test_state_major_odd_tail(gpu, orc, monkeypatch, w4):
    """389 instances state-major (16 candidates per state): 24 whole groups and one of 5; one
    group has a single contact word (15 covered: 7 of its 8 wavefronts leave after the inputs),
    19 have two and 5 three.  Dedup on equals dedup off bit for bit, the counter equals the
    recomputed count (0 with the switch off), and the results match the oracle -- with the
    3-wave build (the default at this size) and the 4-wave one."""
    import mpcqp
    p = mpcqp.model_params("B")
    batch = mpcqp.make_batch(p, 389, seed=91)
    cm = covered_mask(batch, p["N"])
    words = [len(set(batch["contact"][g:g + 16].tolist())) for g in range(0, 389, 16)]
    assert (words.count(1), words.count(2), words.count(3)) == (1, 19, 5) and cm.sum() == 335
    on = run(p, batch, monkeypatch, True, w4)
    off = run(p, batch, monkeypatch, False, w4)
    assert off["covered"] == 0
    assert on["covered"] == int(cm.sum())
    assert_same_bits(on, off)
    assert np.all(on["status"] == 0)
    assert_oracle(orc, p, batch, on)


def test_same_word_different_data(gpu, orc, monkeypatch):
    """64 distinct states, one candidate each, two contact words: every group is full of
    instances that share a word with their leader and differ in the data.  None is covered."""
    import mpcqp
    p = mpcqp.model_params("B")
    batch = mpcqp.make_batch(p, 64, seed=5, candidates=1)
    assert len(set(batch["contact"].tolist())) == 2 and covered_mask(batch, p["N"]).sum() == 0
    on = run(p, batch, monkeypatch, True)
    assert on["covered"] == 0
    assert np.all(on["status"] == 0)
    assert_oracle(orc, p, batch, on)


def test_near_duplicates(gpu, orc, monkeypatch):
    """state-major batch of 64; in every group one follower differs from its leader by one ulp in
    one element of exactly one of x0 / xref / lin (the array rotates over the groups), another
    by the sign of a zero entry of xref, a third by 0.01 in x0[4].  None of the three is
    covered, every other follower is; the shifted instance's U differs from its leader's."""
    import mpcqp
    p = mpcqp.model_params("B")
    batch = {k: v.copy() for k, v in mpcqp.make_batch(p, 64, seed=17).items()}
    batch["xref"][:, 5, 7] = 0.0  # a zero entry, in every candidate of every state
    base = covered_mask(batch, p["N"])
    shifted = []
    for g, g0 in enumerate(range(0, 64, 16)):
        f = [i for i in range(g0, g0 + 16) if base[i]]
        assert len(f) >= 3
        a, b, c = f[0], f[len(f) // 2], f[-1]
        arr, at = (("x0", (a, 6)), ("xref", (a, 3, 9)), ("lin", (a, 2)), ("xref", (a, 0, 0)))[g]
        batch[arr][at] = np.nextafter(batch[arr][at], np.inf)
        batch["xref"][b, 5, 7] = -0.0
        batch["x0"][c, 4] += 0.01
        shifted.append(c)
        touched = {a, b, c}
        cm = covered_mask(batch, p["N"])
        assert not cm[[a, b, c]].any()
        assert all(cm[i] for i in f if i not in touched)
    cm = covered_mask(batch, p["N"])
    assert cm.sum() == base.sum() - 12
    on = run(p, batch, monkeypatch, True)
    off = run(p, batch, monkeypatch, False)
    assert on["covered"] == int(cm.sum()) and off["covered"] == 0
    assert_same_bits(on, off)
    ct = batch["contact"]
    for c in shifted:
        lead = next(j for j in range(c & ~15, c) if ct[j] == ct[c])
        assert not np.array_equal(on["U"][c], on["U"][lead])
    assert_oracle(orc, p, batch, on, np.array(shifted))
    assert_oracle(orc, p, batch, on)


def test_mixed_groups(gpu, orc, monkeypatch):
    """one group of 16 distinct words on one state's data (the stance foot lifted at different
    steps: nothing to cover, ranked as by word alone), one group of 16 identical words (15
    covered) and a short group whose first two instances are the same double-support QP (33
    free forces: both defer to the overflow kernel, neither is covered) beside a plain one."""
    import mpcqp
    p = mpcqp.model_params("B")
    N = p["N"]
    batch = {k: v[:35].copy() for k, v in mpcqp.make_batch(p, 48, seed=29).items()}
    ct = batch["contact"].astype(np.uint64)
    w0 = int(ct[0])
    for i in range(16):
        steps = [] if i == 0 else [i - 1] if i <= 10 else [i - 11, i - 6]
        w = w0
        for k in steps:
            w &= ~(3 << (2 * k))
        ct[i] = np.uint64(w)
    ct[16:32] = ct[16]
    ct[32] = ct[33] = np.uint64(int(ct[32]) | (3 << (2 * 4)))
    batch["contact"] = ct
    assert len(set(ct[:16].tolist())) == 16
    assert 3 * bin(int(ct[32])).count("1") == 33 > PAIR_NF
    cm = covered_mask(batch, N)
    assert cm[:16].sum() == 0 and cm[16:32].sum() == 15 and cm[32:].sum() == 0
    on = run(p, batch, monkeypatch, True)
    off = run(p, batch, monkeypatch, False)
    assert on["covered"] == 15 and off["covered"] == 0
    assert_same_bits(on, off)
    assert np.all(on["status"] == 0)
    assert_oracle(orc, p, batch, on)


def test_literal_model_reports_no_dedup(gpu, monkeypatch):
    """a context whose kernel never covers (the literal model: no contact words to lead by)
    reports no dedup whatever the switch; the SRBM context at N = 10 reports it"""
    import mpcqp
    from mpcqp.engine import BatchEngine
    monkeypatch.delenv("MPCQP_PAIR_DEDUP", raising=False)
    eng = BatchEngine(mpcqp.model_params("L"))
    assert not eng.pair_dedup
    eng.close()
    eng = BatchEngine(mpcqp.model_params("B"))
    assert eng.fused_kernel == "k_mpc_pair" and eng.pair_dedup
    eng.close()


def test_selection_takes_the_leader(gpu, monkeypatch):
    """mpcqp_batch_solve_select on the 389 batch: covered instances commit no key, and their
    leader has the lowest index of its class, so the fused record is the host restatement's bit
    for bit (index_base 0 and 123,457, twice each: the slots and tickets re-arm although most
    wavefronts leave early) and the winner is not a covered instance."""
    import torch
    import mpcqp
    from mpcqp.dist import decode_record, host_record
    from mpcqp.engine import BatchEngine
    monkeypatch.delenv("MPCQP_PAIR_DEDUP", raising=False)
    p = mpcqp.model_params("B")
    nV = p["nu"] * p["N"]
    batch = mpcqp.make_batch(p, 389, seed=91)
    cm = covered_mask(batch, p["N"])
    eng = BatchEngine(p)
    assert eng.pair_dedup
    d = eng.upload(batch)
    dev = torch.device("cuda:0")
    for base in (0, 0, 123_457, 123_457):
        d["U"].fill_(float("nan"))
        d["cost"].fill_(float("nan"))
        d["status"].fill_(99)
        rec = torch.full((1 + nV,), -1, dtype=torch.int64, device=dev)
        eng.solve_select(d, rec, index_base=base)
        eng.sync()
        got = rec.cpu().numpy()
        cost, status, U = (d[k].cpu().numpy() for k in ("cost", "status", "U"))
        assert np.all(status == 0)
        np.testing.assert_array_equal(got, host_record(cost, status, U, base))
        _, gi, _ = decode_record(got)
        assert 0 <= gi - base < 389 and not cm[gi - base]
    eng.close()
