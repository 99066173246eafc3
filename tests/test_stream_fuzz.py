"""Seeded random rounds through the streaming-context batch calls (device mode), checked against hashlib:
a context table of random size, and per round a random subset of it in random order, each named context
taking a piece of 0 .. 300 bytes from a random offset of one shared buffer (pieces overlap freely).  After
3 .. 8 rounds every context is finalised.  The fixed seeds make a failure reproducible."""
import hashlib

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WIDTH = {"md5": 168, "sha1": 92}


@pytest.fixture(scope="module")
def torch_dev(brb):
    import torch
    assert torch.cuda.is_available(), "no HIP device visible to torch"
    assert brb.gpu_available(), brb.lib().BRB_CryptoGPU_LastError()
    return torch


@pytest.mark.parametrize("seed", range(24))
def test_fuzz_streams(brb, torch_dev, seed):
    torch = torch_dev
    rng = np.random.default_rng(0x57E4 + seed)
    alg = ("md5", "sha1")[seed & 1]
    n_ctx = int(rng.integers(1, 2001))
    buf = rng.integers(0, 256, int(rng.integers(301, 20000)), dtype=np.uint8)
    raw = buf.tobytes()
    d_buf = torch.from_numpy(buf).cuda()
    ctxs = torch.full((n_ctx, WIDTH[alg]), 0xEE, dtype=torch.uint8, device="cuda")
    getattr(brb, alg + "_init_batch")(ctxs)
    msgs = [[] for _ in range(n_ctx)]
    for _ in range(int(rng.integers(3, 9))):
        n = int(rng.integers(1, n_ctx + 1))
        idx = rng.permutation(n_ctx)[:n].astype(np.uint32)
        lens = rng.integers(0, 301, n).astype(np.uint32)
        offs = (rng.random(n) * (buf.size - lens + 1)).astype(np.uint64)
        getattr(brb, alg + "_update_batch")(ctxs, d_buf, torch.from_numpy(offs.view(np.int64)).cuda(),
                                            torch.from_numpy(lens.view(np.int32)).cuda(),
                                            ctx_index=torch.from_numpy(idx.view(np.int32)).cuda())
        for c, o, k in zip(idx.tolist(), offs.tolist(), lens.tolist()):
            msgs[c].append(raw[o:o + k])
    order = rng.permutation(n_ctx).astype(np.uint32)
    got = getattr(brb, alg + "_final_batch")(ctxs, ctx_index=torch.from_numpy(order.view(np.int32)).cuda()).cpu().numpy()
    want = [getattr(hashlib, alg)(b"".join(msgs[c])).digest() for c in order.tolist()]
    assert [got[i].tobytes() for i in range(n_ctx)] == want, (alg, n_ctx)
    assert np.array_equal(d_buf.cpu().numpy(), buf)
