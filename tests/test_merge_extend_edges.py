"""lra_merge_extend_batch, lra_trim_overlapped_anchors_batch and lra_trim_anchor_pairs_batch (merge_extend.hip) on the crafted cases of tests/btwn_cases.py:
MergeChain at its distance limits and groupings, members and groups without matches, the tables of skipped slots between live ones, DiagonalSort keys of every sign
and on every chromosome, cluster sizes around the workgroup sort's limits, groups of 63 / 64 / 65 anchors, and the trim walk with anchors given directly.  Group
membership, anchors, lengths, box, strand and chromosome are compared with the oracle exactly."""
import ctypes as C

import numpy as np
import pytest

import btwn_cases as bc

MERGE = [(n, c) for n, c in bc.all_cases() if c["kind"] == "merge"]


def run_merge(ctx, named, **layout):
    from lra_amd import chain
    P = bc.pack(named, **layout)
    dev, ch, sp, rf = bc.to_device(ctx, P)
    bt = chain.BtwnResult(); bt.n_frags = P["n_frags"]; bt.n_matches = P["n_matches"]
    bt.d_match_off = rf.d_match_off; bt.d_match_q = rf.d_match_q; bt.d_match_t = rf.d_match_t; bt.d_box = rf.d_box
    mres = chain.merge_extend_batch(ctx, ch, sp, bt, dev["strands"], dev["read_off"], dev["genome"], bc.CHROM, K=bc.K)
    return P, mres


def check_merge(ctx, named, P, mres):
    from lra_amd import chain
    mo = chain.fetch_merge(ctx, mres)
    live = {P["where"][n][0]: (n, c) for n, c in named}
    groups = clusters = 0
    for s in range(P["n_slots"]):
        g0, g1 = int(mo["slot_group_off"][s]), int(mo["slot_group_off"][s + 1])
        assert g0 == groups and int(mo["cluster_base"][s]) == clusters, ("tables at slot", s, live.get(s, ("skipped",))[0])
        if s not in live:
            assert g1 == g0 and int(mo["cluster_base"][s + 1]) == clusters, ("a skipped slot has groups or clusters", s)
            continue
        n, c = live[s]
        e = bc.oracle_merge(c)
        ng = len(e["member"]) - 1
        assert g1 - g0 == ng, (n, "groups", g1 - g0, ng)
        cb = clusters
        for g in range(ng):
            G = g0 + g
            first, last = (int(e["member"][g]) if g else 0), int(e["member"][g + 1]) - 1
            assert (int(mo["group_first"][G]) - cb, int(mo["group_last"][G]) - cb) == (first, last), (n, g, "members")
            a0, cnt = int(mo["anchor_off"][G]), int(mo["count"][G])
            e0, e1 = int(e["anchor_off"][g]), int(e["anchor_off"][g + 1])
            assert cnt == e1 - e0, (n, g, "anchors", cnt, e1 - e0)
            assert np.array_equal(mo["q"][a0:a0 + cnt], e["q"][e0:e1]) and np.array_equal(mo["t"][a0:a0 + cnt], e["t"][e0:e1]), (n, g, "anchor positions")
            assert np.array_equal(mo["len"][a0:a0 + cnt], e["len"][e0:e1]), (n, g, "anchor lengths")
            assert np.array_equal(mo["box"][G], e["box"][g]), (n, g, "box", mo["box"][G].tolist(), e["box"][g].tolist())
            assert (int(mo["strand"][G]), int(mo["chrom"][G])) == (int(e["strand"][g]), int(e["chrom"][g])), (n, g, "strand / chromosome")
        groups += ng; clusters += len(c["clusters"])
    assert mres.n_groups == groups and int(mo["anchor_off"][groups]) == mres.n_anchors


@pytest.mark.gpu
def test_hip_merge_extend_edges(ctx, oracle):
    """every merge case in one batch: padding fragments, marked slots between live ones, several chains on a read"""
    P, mres = run_merge(ctx, MERGE)
    assert int((P["status"] != 0).sum()) > 3
    check_merge(ctx, MERGE, P, mres)
    rev = MERGE[::-1]
    P, mres = run_merge(ctx, rev, pad=False, marked=False, empty_slots=2)
    check_merge(ctx, rev, P, mres)


@pytest.mark.gpu
def test_hip_merge_extend_nothing_to_do(ctx, oracle):
    """every slot skipped (the early return), and clusters present without a single match"""
    P, mres = run_merge(ctx, MERGE[:6], all_marked=True)
    assert mres.n_groups == 0 and mres.n_anchors == 0
    assert np.all(ctx.to_host(mres.d_slot_group_off, P["n_slots"] + 1, np.uint64) == 0)
    named = [(n, c) for n, c in MERGE if n == "merge.no_matches"]
    P, mres = run_merge(ctx, named, pad=False, marked=False)
    assert P["n_matches"] == 0 and mres.n_anchors == 0
    check_merge(ctx, named, P, mres)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["trim", "trimpairs"])
def test_hip_trim_edges(ctx, oracle, kind):
    """TrimOverlappedAnchors with the anchors given directly: the cluster version (long anchors of 40, both strands) and the pair version (50, forward)"""
    import torch
    named = [(n, c) for n, c in bc.all_cases() if c["kind"] == kind]
    assert len(named) > 15
    off = np.cumsum([0] + [len(c["q"]) for _, c in named]).astype(np.int64)
    cat = lambda f, dt: np.array([v for _, c in named for v in c[f]], dt)
    dq, dt, dl = (torch.from_numpy(cat(f, np.int64).astype(np.uint32).view(np.int32) if f != "len" else cat(f, np.int32)).to(ctx.device) for f in ("q", "t", "len"))
    doff = torch.from_numpy(off).to(ctx.device)
    if kind == "trim":
        dst = torch.tensor([c["strand"] for _, c in named], dtype=torch.int32, device=ctx.device)
        ctx.check(ctx.lib.lra_trim_overlapped_anchors_batch(ctx.h, len(named), doff.data_ptr(), int(off[-1]), dst.data_ptr(), dq.data_ptr(), dt.data_ptr(), dl.data_ptr()))
    else:
        ctx.check(ctx.lib.lra_trim_anchor_pairs_batch(ctx.h, C.c_uint64(len(named)), C.c_void_p(doff.data_ptr()), C.c_uint64(int(off[-1])), C.c_void_p(dq.data_ptr()),
                                                      C.c_void_p(dt.data_ptr()), C.c_void_p(dl.data_ptr())))
    gq = dq.cpu().numpy().view(np.uint32); gl = dl.cpu().numpy()
    for k, (n, c) in enumerate(named):
        eq, el = bc.oracle_trim(c)
        a, b = int(off[k]), int(off[k + 1])
        assert np.array_equal(gl[a:b], np.asarray(el, np.int32)), (n, "lengths", gl[a:b].tolist(), np.asarray(el).tolist())
        assert np.array_equal(gq[a:b], np.asarray(eq, np.uint32)), (n, "read positions")
