"""Clipped Adam under DataParallel, world size 2 (ranks started as tests/test_distributed_cpu.py starts them): gradients
arrive as the SUM over ranks and the global norm takes the optimizer's `grad_scale` = 1 / world, so two ranks on half a batch
each end where one process on the whole batch ends, and both report the same norm.  Once on the `cpu` device over
tests/gloo_comm.py (the array statement, optim/clip.py), once on the emulated HIP device (the fused entries)."""
import os
import sys

import numpy as np
import pytest
import torch.multiprocessing as mp

from tests.test_distributed_cpu import ROOT, _Patch, _free_port

STEPS = 2


def _steps(dev, lo, hi, dp_of=None):
    import pydynet_amd as pdn
    import pydynet_amd.nn.functional as F
    from tests import test_grad_clip as T
    net, _, _ = T.build(dev)
    x = pdn.Tensor(T.X[lo:hi], dtype=np.float32, device=dev)
    y = pdn.Tensor(T.Y[lo:hi], dtype=np.int64, device=dev)
    opt = T.clipped_adam(list(net.parameters()))
    dp = dp_of(net, opt) if dp_of else None
    norms = []
    for _ in range(STEPS):
        opt.zero_grad()
        F.cross_entropy_loss(net(x), y).backward()
        if dp is not None:
            dp.finish()
        opt.step()
        norms.append(float(T.host(opt.last_grad_norm)))
    return [p.numpy() for p in net.parameters()], norms


def _worker(rank, world, port, out_dir, dev):
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    from pydynet_amd import _lib, distributed as pdist
    from pydynet_amd.distributed import DataParallel, init_process_group, shard_batch
    if dev == "cpu":
        from tests import gloo_comm
        gloo_comm.install()
        init_process_group("gloo")
    else:
        from tests import abi_emulator
        abi_emulator.install(_Patch())
        init_process_group("rccl", 0)
    lo, hi = shard_batch(16, rank, world)
    params, norms = _steps(dev, lo, hi, lambda net, opt: DataParallel(net, opt, bucket_mb=0.05))
    if dev != "cpu":
        calls = _lib.lib().calls
        assert calls.count("pdnx_grad_norm_multi_f32") == STEPS and calls.count("pdnx_adam_multi_clip_f32") == STEPS
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), norms=np.array(norms), **{f"p{i}": p for i, p in enumerate(params)})
    pdist.get_group().barrier()
    pdist.destroy_process_group()


def _check(tmp_path, dev):
    from tests.test_grad_clip import MAX_NORM
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path), dev), nprocs=2, join=True)
    r0, r1 = (np.load(tmp_path / f"rank{r}.npz") for r in range(2))
    ref_params, ref_norms = _steps(dev, 0, 16)
    assert np.array_equal(r0["norms"], r1["norms"]) and (r0["norms"] > MAX_NORM).all()
    assert np.allclose(r0["norms"], ref_norms, rtol=1e-5), (r0["norms"], ref_norms)
    for i, p in enumerate(ref_params):
        assert np.array_equal(r0[f"p{i}"], r1[f"p{i}"])
        assert np.allclose(r0[f"p{i}"], p, rtol=1e-4, atol=2e-6), (i, float(np.abs(r0[f"p{i}"] - p).max()))


def test_two_ranks_with_clipping_equal_the_single_process_step(tmp_path):
    _check(tmp_path, "cpu")


def test_two_ranks_with_clipping_on_the_emulated_hip_device(tmp_path, emulated_hip):
    _check(tmp_path, "hip:0")
