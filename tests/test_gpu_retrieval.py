"""GPU: the retrieval kernels (csrc/retrieval.hip) and RetrievalDatabase against a float64 oracle restated from the
reference text (mast3r_utils.py:696-715 signature, :738-768 / :784-795 top-k): signature = mean over tokens,
/ sqrt(sum x^2 + 1e-8); similarity = dot product; order = reversed stable ascending argsort; update keeps sim > thresh."""
import types

import numpy as np
import pytest
import torch

from mast3r_slam import _ffi, model as M, retrieval, synthetic
from mast3r_slam.frame import create_frame

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- oracle (float64)
def sig_oracle(feat):
    x = feat.detach().cpu().double().numpy()
    x = x.reshape(-1, x.shape[-2], x.shape[-1]) if x.ndim > 1 else x.reshape(1, 1, -1)
    m = x.mean(axis=1)
    return m / np.sqrt((m * m).sum(axis=1, keepdims=True) + 1e-8)


def topk_oracle(q, db, lim, k, thresh=None):
    sims = db[:lim].astype(np.float64) @ q.astype(np.float64)
    order = np.argsort(sims, kind="stable")[::-1][:min(k, lim)]
    if thresh is not None:
        order = [i for i in order if sims[i] > thresh]
    return [int(i) for i in order], [float(sims[i]) for i in order]


def topk(q, db, N, k, thresh=None, causal=False):
    """The C entry point directly: q [Q,C], db [rows,C] fp32 on the device."""
    Q, C = q.shape
    L = _ffi.lib()
    ws = torch.empty((max(L.m3_retrieval_ws_bytes(N, Q, k, int(causal)), 16),), dtype=torch.uint8, device=q.device)
    count = torch.full((Q,), -7, dtype=torch.int32, device=q.device)
    idx = torch.empty((Q, k), dtype=torch.int32, device=q.device)
    score = torch.empty((Q, k), dtype=torch.float32, device=q.device)
    _ffi.call("m3_retrieval_topk", q.data_ptr(), q.stride(0), db.data_ptr(), db.stride(0), N, Q, C, k,
              int(thresh is not None), float(thresh or 0.0), int(causal), count.data_ptr(), idx.data_ptr(),
              score.data_ptr(), ws.data_ptr(), ws.numel(), _ffi.stream_ptr())
    return count.cpu().numpy(), idx.cpu().numpy(), score.cpu().numpy()


def unit_rows(n, c, seed):
    x = np.random.default_rng(seed).normal(size=(n, c))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32)


# ---------------------------------------------------------------- signature
@pytest.mark.parametrize("dtype", [torch.float16, torch.bfloat16, torch.float32])
@pytest.mark.parametrize("T", [1, 441, 672, 1024])
@pytest.mark.parametrize("C", [8, 1024])
def test_signature_matches_float64_oracle(dev, dtype, T, C):
    g = torch.Generator().manual_seed(T * 7 + C)
    feat = (torch.randn(4, T, C, generator=g) + 0.3 * torch.randn(1, 1, C, generator=g))
    feat[2] = (torch.arange(C) % 7 - 3).float() * 3e-7                   # constant row: the norm is the 1e-8's
    feat[3] = 0.0                                                          # all zero: the signature is exactly 0
    feat = feat.to(dtype).to(dev)
    db = retrieval.RetrievalDatabase(None, backbone_dim=C)
    sig = db.compute_signature(feat)
    assert sig.shape == (4, C) and sig.dtype == torch.float32 and sig.is_cuda
    ref = sig_oracle(feat)
    got = sig.cpu().double().numpy()
    assert np.abs(got - ref).max() <= 1e-6
    rel = np.linalg.norm(got[:3] - ref[:3]) / np.linalg.norm(ref[:3])
    assert rel <= 1e-6
    ss = (feat[2, 0].double().cpu() ** 2).sum().item()
    assert ss < 1e-8 and np.abs(got[2]).max() > 1e-3                        # the constant row is not all-zero
    assert torch.equal(sig[3], torch.zeros(C, device=dev))
    # [T,C] and [C] inputs
    one = db.compute_signature(feat[0])
    assert one.shape == (C,) and torch.equal(one, sig[0])
    v = db.compute_signature(feat[0, 0])
    assert np.abs(v.cpu().double().numpy() - sig_oracle(feat[0, 0])[0]).max() <= 1e-6


@pytest.mark.parametrize("T", [441, 1024])
def test_signature_bits_do_not_depend_on_the_batch(dev, T):
    C = 1024
    feat = torch.randn(8, T, C, generator=torch.Generator().manual_seed(T)).to(torch.float16).to(dev)
    db = retrieval.RetrievalDatabase(None, backbone_dim=C)
    batch = db.compute_signature(feat)
    for b in range(8):
        assert torch.equal(db.compute_signature(feat[b]), batch[b]), b
    # written at a strided destination row: the same bits
    out = torch.full((8, 2 * C), 5.0, device=dev)
    db._signatures_into(feat.contiguous(), out[:, C // 2:C // 2 + C])
    assert torch.equal(out[:, C // 2:C // 2 + C], batch) and bool((out[:, :C // 2] == 5).all())


# ---------------------------------------------------------------- top-k
@pytest.mark.parametrize("C", [64, 1024])
def test_topk_matches_oracle_and_batched_queries_are_bitwise(dev, C):
    N, Q = 1000, 8
    dbh = unit_rows(N + 8, C, 1)
    qh = unit_rows(Q, C, 2)
    db, q = torch.from_numpy(dbh).to(dev), torch.from_numpy(qh).to(dev)
    for k in (1, 3, 5):
        cnt, idx, sc = topk(q, db, N, k)
        for i in range(Q):
            ro, so = topk_oracle(qh[i], dbh, N, k)
            sims = dbh[:N].astype(np.float64) @ qh[i].astype(np.float64)
            assert cnt[i] == k and np.abs(sc[i] - so).max() <= 1e-5
            for j in range(k):                                              # same order, except inside an fp32 near-tie
                assert idx[i, j] == ro[j] or abs(sims[idx[i, j]] - so[j]) < 1e-6, (i, j)
        for i in range(Q):                                                  # Q = 8 equals eight Q = 1 calls, bitwise
            c1, i1, s1 = topk(q[i:i + 1], db, N, k)
            assert c1[0] == cnt[i] and np.array_equal(i1[0], idx[i]) and np.array_equal(s1[0].view(np.int32),
                                                                                         sc[i].view(np.int32))
    # growing N leaves every score's bits alone
    _, i_a, s_a = topk(q[:1], db, 300, 64)
    _, i_b, s_b = topk(q[:1], db, N, 64)
    sa = dict(zip(i_a[0].tolist(), s_a[0].tolist()))
    common = [(i, s) for i, s in zip(i_b[0].tolist(), s_b[0].tolist()) if i in sa]
    assert common and all(sa[i] == s for i, s in common)


def test_topk_ties_threshold_and_small_databases(dev):
    C = 8
    rows = np.zeros((8, C), np.float32)
    rows[:, 0] = [0.25, 0.5, 0.5, 0.125, 0.25 + 2.0 ** -20, 0.5, -0.25, 0.0]   # exact products with e0
    db = torch.from_numpy(rows).to(dev)
    q = torch.zeros((1, C), device=dev)
    q[0, 0] = 1.0
    # ties (rows 1, 2, 5 score 0.5 exactly): the larger index first
    cnt, idx, sc = topk(q, db, 8, 4)
    assert cnt[0] == 4 and idx[0].tolist() == [5, 2, 1, 4] and sc[0].tolist()[:3] == [0.5, 0.5, 0.5]
    assert idx[0].tolist() == topk_oracle(q[0].cpu().numpy(), rows, 8, 4)[0]
    # a score exactly at the threshold is excluded (sim > min_thresh)
    cnt, idx, sc = topk(q, db, 8, 8, thresh=0.25)
    assert cnt[0] == 4 and idx[0].tolist()[:4] == [5, 2, 1, 4] and idx[0].tolist()[4:] == [-1] * 4
    cnt, idx, _ = topk(q, db, 8, 8, thresh=0.0)
    assert cnt[0] == 6 and 7 not in idx[0].tolist()[:6] and 6 not in idx[0].tolist()[:6]
    # identical rows tie exactly on random data too
    dbh = unit_rows(600, 64, 3)
    dbh[500] = dbh[10]
    qh = dbh[10:11].copy()
    cnt, idx, sc = topk(torch.from_numpy(qh).to(dev), torch.from_numpy(dbh).to(dev), 600, 3)
    assert idx[0].tolist()[:2] == [500, 10] and sc[0, 0] == sc[0, 1]
    assert idx[0].tolist() == topk_oracle(qh[0], dbh, 600, 3)[0]
    # k > N, N = 0, k = 1
    cnt, idx, _ = topk(q, db, 2, 5)
    assert cnt[0] == 2 and idx[0].tolist() == [1, 0, -1, -1, -1]
    cnt, idx, _ = topk(q, db, 0, 3)
    assert cnt[0] == 0 and idx[0].tolist() == [-1, -1, -1]
    cnt, idx, sc = topk(q, db, 8, 1)
    assert cnt[0] == 1 and idx[0].tolist() == [5] and sc[0, 0] == 0.5


def test_topk_causal_rows(dev):
    """causal = 1: query q sees rows [0, N + q) - the batched update's view of the database."""
    C, N, Q = 64, 40, 8
    dbh = unit_rows(N + Q, C, 4)
    dbh[N + 3] = dbh[N + 1]                                                # query 3 must find row N + 1 (inserted before it)
    db = torch.from_numpy(dbh).to(dev)
    cnt, idx, sc = topk(db[N:], db, N, 3, thresh=-2.0, causal=True)
    for i in range(Q):
        ro, so = topk_oracle(dbh[N + i], dbh, N + i, 3, thresh=-2.0)
        assert idx[i].tolist()[:cnt[i]] == ro and np.abs(sc[i, :cnt[i]] - so).max() <= 1e-5
    assert idx[3, 0] == N + 1


# ---------------------------------------------------------------- database
def _fake(feat):
    return types.SimpleNamespace(feat=feat)


def test_growth_keeps_rows_and_scores_bitwise(dev):
    C, T = 64, 16
    g = torch.Generator().manual_seed(9)
    feats = torch.randn(1000, T, C, generator=g).to(torch.float16).to(dev)
    db = retrieval.RetrievalDatabase(None, backbone_dim=C)
    snap, scores = None, []
    for lo, hi in ((0, 1), (1, 63), (63, 64), (64, 65), (65, 1000)):
        db.update_batch([_fake(feats[i]) for i in range(lo, hi)])
        assert len(db) == hi and db.kf_counter == hi and db.kf_ids == list(range(hi)) and db.capacity >= hi
        if snap is None:
            snap = db.signatures[:1].clone()
        assert torch.equal(db.signatures[:1], snap)
        ids, sc = db.query(feats[0], k=1)
        assert ids == [0]
        scores.append(sc[0])
    assert db.capacity == 1024 and len(set(scores)) == 1
    assert torch.equal(db.signatures, db.compute_signature(feats))


@pytest.mark.parametrize("add_after_query", [True, False])
def test_update_batch_equals_sequential_updates(dev, add_after_query):
    C, T = 64, 32
    feats = torch.randn(11, T, C, generator=torch.Generator().manual_seed(5)).to(torch.bfloat16).to(dev)
    feats[9] = feats[6]                                                     # a repeat inside the batch
    feats[10] = feats[1]                                                    # a repeat of a stored frame
    a, b = (retrieval.RetrievalDatabase(None, backbone_dim=C) for _ in range(2))
    for i in range(5):
        assert a.update(_fake(feats[i]), k=3, min_thresh=-1.0) == b.update(_fake(feats[i]), k=3, min_thresh=-1.0)
    seq = [a.update(_fake(feats[i]), add_after_query=add_after_query, k=3, min_thresh=0.005) for i in range(5, 11)]
    bat = b.update_batch([_fake(feats[i]) for i in range(5, 11)], add_after_query=add_after_query, k=3,
                         min_thresh=0.005)
    assert seq == bat and len(a) == len(b) and a.kf_ids == b.kf_ids and a.kf_counter == b.kf_counter
    assert torch.equal(a.signatures, b.signatures)
    assert seq[5][0] == 1
    if add_after_query:
        assert seq[4][0] == 6 and len(a) == 11
    else:
        assert len(a) == 5


def test_update_on_a_real_frame(dev):
    net = M.Mast3rFull(weights=M.init_random_weights(M.TINY_CFG, seed=1), cfg=M.TINY_CFG, device=dev)
    db = retrieval.load_retriever(net)
    assert db.backbone_dim == 1024
    mk = lambda seed: create_frame(seed, torch.from_numpy(synthetic.textured_image(128, 256, seed)).to(dev))
    f0, f1 = mk(40), mk(41)
    assert db.update(f0) == [] and f0.feat is not None and len(db) == 1
    ref = sig_oracle(f0.feat)[0]
    assert np.abs(db.signatures[0].cpu().double().numpy() - ref).max() <= 1e-6
    assert db.update(f0, add_after_query=False) == [0] and len(db) == 1   # queried, not inserted
    got = db.update(f1, add_after_query=True, k=3, min_thresh=-1.0)
    assert got == [0] and len(db) == 2                                      # never itself
    ids, sc = db.query(f0.feat, k=3)
    assert ids[0] == 0 and abs(sc[0] - 1.0) < 1e-5 and len(ids) == 2
