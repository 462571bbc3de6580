"""CPU: the keyframe retrieval database keeps the reference's names and defaults (mast3r_utils.py:83-114, :640-795),
its C entry points reject bad arguments before any HIP call, CPU tensors fail loudly, Keyframes.pop_last, and the
SLAM driver's new arguments default to the old behaviour."""
import inspect

import pytest
import torch

from mast3r_slam import _ffi, mast3r_utils, retrieval
from mast3r_slam.frame import Keyframes, create_frame


def _params(fn):
    sig = inspect.signature(fn).parameters
    return [(k, sig[k].default) for k in sig]


def test_reference_names_parameters_and_defaults():
    E = inspect.Parameter.empty
    assert mast3r_utils.load_retriever is retrieval.load_retriever
    assert mast3r_utils.RetrievalDatabase is retrieval.RetrievalDatabase
    assert _params(retrieval.load_retriever) == [("model", E), ("backbone_dim", None)]                    # :83-86
    D = retrieval.RetrievalDatabase
    assert _params(D.__init__) == [("self", E), ("model", E), ("backbone_dim", 1024)]                     # :651-655
    assert _params(D.update) == [("self", E), ("frame", E), ("add_after_query", True), ("k", 3), ("min_thresh", 0.0)]
    assert _params(D.query) == [("self", E), ("features", E), ("k", 3)]                                   # :770
    assert _params(D.compute_signature) == [("self", E), ("features", E)]
    assert callable(D.prep_features) and callable(D.update_batch)


class _Model:
    embed_dim = 64


def test_database_without_a_device():
    db = retrieval.load_retriever(_Model())
    assert db.backbone_dim == 64 and db.use_simple_retrieval is True
    assert len(db) == 0 and db.kf_ids == [] and db.kf_counter == 0 and db.signatures.shape == (0, 64)
    assert retrieval.load_retriever(_Model(), backbone_dim=32).backbone_dim == 32
    assert retrieval.load_retriever(object()).backbone_dim == 1024
    with pytest.raises(NotImplementedError, match="retrieval head"):
        db.prep_features(torch.zeros(4, 64))
    assert db.query(torch.zeros(4, 64)) == ([], [])                        # empty database: nothing to compare


def test_cpu_tensors_fail_loudly():
    db = retrieval.RetrievalDatabase(None, backbone_dim=64)
    for x in (torch.zeros(4, 64), torch.zeros(2, 4, 64), torch.zeros(64), torch.zeros(4, 64, dtype=torch.float16)):
        with pytest.raises(RuntimeError, match="ROCm device"):
            db.compute_signature(x)
    f = create_frame(0, torch.zeros(32, 32, 3, dtype=torch.uint8), T_WC=torch.zeros(1, 8))
    f.feat = torch.zeros(4, 64, dtype=torch.float16)
    with pytest.raises(RuntimeError, match="ROCm device"):
        db.update(f)
    assert len(db) == 0 and db.kf_counter == 0


def test_entry_points_reject_invalid_arguments_without_a_gpu():
    L = _ffi.lib()
    fake = 1 << 20                                                          # never dereferenced: validation comes first
    ws = 1 << 40
    # signature: NULLs, C not a multiple of 8, T < 1, bad dtype, short stride / workspace, misaligned input
    assert L.m3_retrieval_signature(None, fake, 16, fake, ws, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, None, 16, fake, ws, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 16, None, ws, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 12, fake, ws, 1, 4, 12, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 16, fake, ws, 1, 0, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 16, fake, ws, 0, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 16, fake, ws, 1, 4, 16, 2, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 8, fake, ws, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake, fake, 16, fake, 4, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature(fake + 2, fake, 16, fake, ws, 1, 4, 16, 1, None) == -1
    assert L.m3_retrieval_signature_ws_bytes(2, 33, 16) == 2 * 2 * 16 * 4
    assert L.m3_retrieval_signature_ws_bytes(1, 4, 12) == 0
    # top-k: k = 0 / 65, C % 8, NULLs, N < 0, Q < 1, short strides, bad flags, short workspace
    args = lambda **o: [o.get(n, d) for n, d in (
        ("q", fake), ("ldq", 16), ("db", fake), ("ldd", 16), ("N", 10), ("Q", 1), ("C", 16), ("k", 3), ("th", 1),
        ("thr", 0.0), ("causal", 0), ("count", fake), ("idx", fake), ("score", fake), ("ws", fake), ("wsb", ws),
        ("stream", None))]
    assert L.m3_retrieval_ws_bytes(10, 1, 3, 0) > 0
    for bad in (dict(k=0), dict(k=65), dict(C=12, ldq=12, ldd=12), dict(q=None), dict(db=None), dict(count=None),
                dict(idx=None), dict(score=None), dict(ws=None), dict(N=-1), dict(Q=0), dict(ldq=8), dict(ldd=8),
                dict(ldd=18), dict(th=2), dict(causal=2), dict(wsb=8), dict(db=fake + 4)):
        assert L.m3_retrieval_topk(*args(**bad)) == -1, bad
    assert L.m3_retrieval_ws_bytes(10, 1, 0, 0) == 0 and L.m3_retrieval_ws_bytes(10, 1, 65, 0) == 0
    with pytest.raises(RuntimeError, match="invalid argument"):
        _ffi.call("m3_retrieval_topk", *args(k=65))
    assert L.m3_abi_version() == 4000                                      # the retrieval symbols came with ABI 3; 4000 removed the one-group conv entry points


def test_keyframes_pop_last():
    kf = Keyframes()
    assert kf.pop_last() is None and len(kf) == 0
    a = create_frame(0, torch.zeros(16, 16, 3, dtype=torch.uint8), T_WC=torch.zeros(1, 8))
    b = create_frame(1, torch.zeros(16, 16, 3, dtype=torch.uint8), T_WC=torch.zeros(1, 8))
    kf.append(a)
    kf.append(b)
    assert kf.pop_last() is b and len(kf) == 1 and kf.last_keyframe() is a
    assert kf.pop_last() is a and kf.pop_last() is None and len(kf) == 0


def test_slam_defaults_keep_the_old_driver():
    from mast3r_slam.slam import SLAM
    p = inspect.signature(SLAM.__init__).parameters
    assert list(p) == ["self", "model", "K", "retrieval", "loop_closure"]
    assert p["K"].default is None and p["retrieval"].default is None and p["loop_closure"].default is False
