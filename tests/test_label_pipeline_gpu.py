"""The training-side label pipeline on the device against label_pipeline_refs.py, bit for bit: every arm of aldi_box_match's dispatch on
every scene (thresholds hit exactly, ties, the low-quality rule, culling, GT lists longer than a 256-entry tile, box_count / box_stride_n),
aldi_compact_labels across its segment sizes, aldi_rpn_apply_sample, aldi_roi_prepare_lists against the oracle's labelling, aldi_roi_gather.
No tolerance anywhere: integers with torch.equal, IoUs by their fp32 bit patterns."""
import pytest
import torch

import label_pipeline_refs as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENT = -7


@pytest.fixture(autouse=True)
def _reset_tuning():
    from aldi_amd import _lib as L
    L.reset_tuning()
    yield
    L.reset_tuning()


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------
# A: the matcher
# ------------------------------------------------------------------------------------------------
_dev_ops, _arm_out = {}, {}


def _device_operands(name, big):
    if (name, big) not in _dev_ops:
        boxes, L, cnt, gt, gcnt = R.operands(R.scene(name), big)
        _dev_ops[(name, big)] = (boxes.float().to(DEV), L, cnt, None if cnt is None else torch.tensor(cnt, dtype=torch.int32, device=DEV),
                                 gt.float().to(DEV), gcnt, torch.tensor(gcnt, dtype=torch.int32, device=DEV))
    return _dev_ops[(name, big)]


@pytest.mark.parametrize("name,arm", [(n, a) for n in R.SCENES for a in R.arms_for(R.scene(n))])
def test_box_match_arm_equals_both_references(name, arm):
    from aldi_amd import _lib as Lib
    from aldi_amd import ops
    sc = R.scene(name)
    big, padded, mw = R.ARMS[arm]
    boxes, L, cnt, cntd, gt, gcnt, gcntd = _device_operands(name, big)
    N, Gmax = sc.N, sc.gmax
    if mw is not None:
        Lib.set_tuning("match_wave", mw)
    for cfg in sc.configs:
        best_iou = torch.full((N, L), float(SENT), device=DEV)
        best_idx = torch.full((N, L), SENT, dtype=torch.int32, device=DEV)
        labels = torch.full((N, L), SENT, dtype=torch.int32, device=DEV)
        scratch = ops.box_match_scratch(N, Gmax, DEV) if padded else torch.empty(N, Gmax, dtype=torch.int32, device=DEV)
        scratch.fill_(0x55555555)
        assert R.select_arm(L, N, Gmax, scratch.numel() * 4, Lib.get_tuning("match_wave")) == arm
        ops.box_match(boxes, boxes.shape[1], cntd, L, gt, gcntd, Gmax, N, cfg[0], cfg[1], cfg[2], best_iou, best_idx, scratch, labels)
        torch.cuda.synchronize()
        got = (best_iou.cpu(), best_idx.cpu(), labels.cpu())
        for which, refs in zip(("integer", "oracle"), R.references(name, big, cfg)):
            for n, (r_iou, r_idx, r_lab) in enumerate(refs):
                c = L if cnt is None else cnt[n]
                where = (name, arm, cfg, which, n)
                assert torch.equal(got[2][n, :c].long(), r_lab), where
                assert torch.equal(got[1][n, :c].long(), r_idx), where
                if gcnt[n] > 0:
                    assert torch.equal(_bits(got[0][n, :c]), _bits(r_iou)), where
                else:
                    assert bool((got[2][n, :c] == 0).all()) and bool((got[1][n, :c] == 0).all()), where
                # padding slots: label -2, IoU and index untouched
                assert bool((got[2][n, c:] == -2).all()) and bool((got[1][n, c:] == SENT).all()) and bool((got[0][n, c:] == float(SENT)).all()), where
        # all arms of one layout agree in every word (the IoU of images without GT included)
        first = _arm_out.setdefault((name, big, cfg), (arm, got))
        assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(got, first[1])), (name, arm, "vs", first[0], cfg)


# ------------------------------------------------------------------------------------------------
# B: lists and gathers
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bg,K", [(0, 1), (8, 8)])
@pytest.mark.parametrize("L", R.COMPACT_L)
def test_compact_labels_lists_equal_nonzero(L, bg, K):
    from aldi_amd import ops
    kinds = R.LABEL_PATTERNS
    for i, kind in enumerate(kinds):
        lab = torch.stack([R.label_pattern(kind, L, bg, K), R.label_pattern(kinds[(i + 3) % len(kinds)], L, bg, K)])
        lists = torch.full((2, 2, L), SENT, dtype=torch.int32, device=DEV)
        counts = torch.full((2, 2), SENT, dtype=torch.int32, device=DEV)
        ops.compact_labels(lab.to(DEV), L, 2, bg, lists, counts)
        torch.cuda.synchronize()
        lists, counts = lists.cpu(), counts.cpu()
        for n in range(2):
            for k, ref in enumerate(R.compact_ref(lab[n], bg)):
                assert int(counts[n, k]) == ref.numel(), (kind, n, k)
                assert torch.equal(lists[n, k, :ref.numel()].long(), ref), (kind, n, k)
                assert bool((lists[n, k, ref.numel():] == SENT).all()), (kind, n, k)


def test_rpn_apply_sample_writes_the_selection_and_nothing_else():
    from aldi_amd import ops
    L, N, S = 5000, 2, 4000
    lab = torch.stack([R.label_pattern("alternating", L, 0, 1), R.label_pattern("segment_firsts", L, 0, 1)])
    lists = torch.full((N, 2, L), 1, dtype=torch.int32)          # entries past the counts: an index that WOULD flip a label
    cnt = []
    for n in range(N):
        pos, neg = R.compact_ref(lab[n], 0)
        lists[n, 0, :pos.numel()], lists[n, 1, :neg.numel()] = pos.int(), neg.int()
        cnt.append((pos.numel(), neg.numel()))
    assert cnt == [(2500, 2500), (1, 1)] and S > max(max(c) for c in cnt)
    g = torch.Generator().manual_seed(2)
    cases = []
    for nsel in ([(0, 0), (0, 0)], [(7, 0), (1, 0)], [(2, 2), (1, 1)], [(128, 128), (0, 1)], [(2500, 2500), (1, 1)]):
        sel = torch.full((N, 2, S), 1, dtype=torch.int32)
        for n in range(N):
            for k in range(2):
                m = nsel[n][k]
                perm = torch.randperm(cnt[n][k], generator=g)[:m].int()
                if m >= 2:
                    perm[0], perm[1] = 0, cnt[n][k] - 1                # the first and the last entry of the list
                    perm[2:] = torch.randperm(cnt[n][k] - 2, generator=g)[:m - 2].int() + 1
                sel[n, k, :m] = perm
        cases.append((torch.tensor(nsel, dtype=torch.int32), sel))
    out = torch.full((N, L), SENT, dtype=torch.int32, device=DEV)      # ONE buffer for all calls: nothing of an earlier selection may stay
    listsd = lists.to(DEV)
    for nsel, sel in cases:
        ops.rpn_apply_sample(out, L, N, listsd, sel.to(DEV), nsel.to(DEV), S)
        torch.cuda.synchronize()
        ref = torch.full((N, L), -1, dtype=torch.int32)
        for n in range(N):
            ref[n, lists[n, 0][sel[n, 0, :int(nsel[n, 0])].long()].long()] = 1
            ref[n, lists[n, 1][sel[n, 1, :int(nsel[n, 1])].long()].long()] = 0
        assert int((ref[0] != -1).sum()) == int(nsel[0].sum())
        assert torch.equal(out.cpu(), ref), nsel.tolist()


@pytest.mark.parametrize("P,Gmax", [(13, 1), (37, 256), (251, 6)])
def test_roi_prepare_lists_equals_the_oracles_labelling(P, Gmax):
    from aldi_amd import ops
    sc = R.roi_scene(P, Gmax)
    ref = R.roi_prepare_ref(sc)
    N, K, L = sc["N"], sc["K"], P + Gmax
    i32 = dict(dtype=torch.int32, device=DEV)
    props, gt = sc["props"].float().to(DEV), sc["gt"].float().to(DEV)
    pcount, gcount, gcls = torch.tensor(sc["pcount"], **i32), torch.tensor(sc["gcount"], **i32), sc["gcls"].to(**i32)
    cand = torch.full((N, L, 4), float(SENT), device=DEV)
    best_iou = torch.full((N, L), float(SENT), device=DEV)
    ccount, best_idx, labels, cls = (torch.full(s, SENT, **i32) for s in ((N,), (N, L), (N, L), (N, L)))
    lists, counts = torch.full((N, 2, L), SENT, **i32), torch.full((2 * N + 2,), SENT, **i32)
    tickets, tail_a, tail_b = torch.zeros(N, **i32), torch.tensor([41], **i32), torch.tensor([43], **i32)
    outs = (cand, ccount, best_iou, best_idx, labels, cls, lists, counts, tickets)

    def call():
        ops.roi_prepare_lists(props, pcount, P, gt, gcls, gcount, Gmax, N, K, 0.5, cand, ccount, best_iou, best_idx, labels, cls, lists, counts, tickets,
                              tail_a, tail_b)
        torch.cuda.synchronize()
        return [t.cpu().clone() for t in outs]
    first = call()
    c_cand, c_count, c_iou, c_idx, c_lab, c_cls, c_lists, c_counts, c_tick = first
    assert bool((c_tick == 0).all())
    for n, r in enumerate(ref):
        c, gc = r["count"], sc["gcount"][n]
        assert int(c_count[n]) == c
        assert torch.equal(c_cand[n, :c], r["cand"].reshape(-1, 4)) and bool((c_cand[n, c:] == 0).all())
        assert torch.equal(c_idx[n, :c].long(), r["midx"]) and bool((c_idx[n, c:] == SENT).all())
        if gc > 0:
            assert torch.equal(_bits(c_iou[n, :c]), _bits(r["best"]))
        assert bool((c_iou[n, c:] == float(SENT)).all())
        assert torch.equal(c_lab[n, :c].long(), r["lab"]) and bool((c_lab[n, c:] == -2).all())
        assert torch.equal(c_cls[n, :c].long(), r["cls"]) and bool((c_cls[n, c:] == -2).all())
        for k, lst in enumerate((r["fg"], r["bg"])):
            assert int(c_counts[2 * n + k]) == lst.numel()
            assert torch.equal(c_lists[n, k, :lst.numel()].long(), lst) and bool((c_lists[n, k, lst.numel():] == SENT).all())
    assert c_counts[2 * N:].tolist() == [41, 43]
    second = call()                                                    # the tickets were left zero: the same again, on the same buffers
    assert all(torch.equal(_bits(a), _bits(b)) for a, b in zip(first, second))


def test_roi_gather_rows_and_nothing_else():
    from aldi_amd import ops
    g = torch.Generator().manual_seed(4)
    N, L, S, Gmax = 4, 77, 9, 5
    cand = torch.randint(0, 500, (N, L, 4), generator=g).float()
    cls = torch.randint(0, 9, (N, L), generator=g).int()
    best_idx = torch.randint(0, Gmax, (N, L), generator=g).int()
    gt = torch.randint(0, 500, (N, Gmax, 4), generator=g).float()
    gcount = [2, 0, 5, 1]                                              # image 1 has no GT: its r_gt rows are zero
    best_idx[3] = 0
    best_idx[0] %= 2
    lists = torch.stack([torch.stack([torch.randperm(L, generator=g)[:40].sort().values, torch.randperm(L, generator=g)[:40].sort().values])
                         for _ in range(N)]).int()
    lists = torch.cat([lists, torch.full((N, 2, L - 40), 1, dtype=torch.int32)], 2)
    nsel = torch.tensor([[0, 5], [4, 0], [3, 6], [S, S]], dtype=torch.int32)          # nf = 0, nb = 0, both, both full
    sel = torch.stack([torch.stack([torch.randperm(40, generator=g)[:S], torch.randperm(40, generator=g)[:S]]) for _ in range(N)]).int()
    sel[3, 0, 0], sel[3, 1, S - 1] = 0, 39
    row_off = torch.tensor([2, 2 + 5 + 3, 2 + 5 + 3 + 4, 30], dtype=torch.int32)      # gaps before image 0, after image 0 and before image 3
    Rr = 30 + 2 * S + 4
    i32 = dict(dtype=torch.int32, device=DEV)
    rois, r_gt = torch.full((Rr, 5), float(SENT), device=DEV), torch.full((Rr, 4), float(SENT), device=DEV)
    r_cls, r_idx = torch.full((Rr,), SENT, **i32), torch.full((Rr,), SENT, **i32)
    ops.roi_gather(cand.to(DEV), cls.to(DEV), best_idx.to(DEV), L, lists.to(DEV), sel.to(DEV), nsel.to(DEV), S, row_off.to(DEV), gt.to(DEV),
                   torch.tensor(gcount, **i32), Gmax, N, rois, r_cls, r_gt, r_idx)
    torch.cuda.synchronize()
    ref = R.roi_gather_ref(cand, cls, best_idx, lists, sel, nsel, row_off, gt, gcount, Rr, float(SENT))
    assert int((ref[3] == SENT).sum()) == Rr - int(nsel.sum()) > 0
    assert bool((ref[2][10:14] == 0).all())
    assert torch.equal(_bits(rois.cpu()), _bits(ref[0])) and torch.equal(_bits(r_gt.cpu()), _bits(ref[2]))
    assert torch.equal(r_cls.cpu().long(), ref[1]) and torch.equal(r_idx.cpu().long(), ref[3])
