"""The gradient guard in a data-parallel job (two gloo ranks, x86 emulation build): every rank computes the norm of the same
all-reduced segment, so the ranks clip and skip alike and stay bit-identical."""
import os

import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import grad_guard_cases as C
from cc_amd import trainer as T
from hipemu.emu import emulated_engine


def _free_port():
    import socket
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def _worker(rank, world, port, ret):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    with emulated_engine():
        nets = C.four_nets("cpu")
        opt = T.FlatAdam(nets, T.StepConfig(max_grad_norm=C.INF))
        opt.broadcast_from_rank0()
        out = []
        for s in range(3):
            # rank-specific shards; step 1: only RANK 1's gradient of PoseNet holds a NaN -- the sum does on both ranks
            C.backward(opt, nets, "cpu", 10 * s + rank, poison=1 if (s == 1 and rank == 1) else None)
            if s == 0:
                own = [float(opt.flat_g[slice(*opt.segment(i))].double().norm()) for i in range(4)]
            if s == 2:      # clip DispNet to half the norm of the mean gradient it just had (the same number on both ranks)
                opt.set_hyper("disp", max_grad_norm=0.5 * float(out[-1]["guard"][0, 0]))
            for i in range(4):              # the per-network form: exchange a segment, then its guarded update
                lo, hi = opt.segment(i)
                opt.all_reduce(lo, hi)
                opt.step_segment(lo, hi, i == 0, opt.grad_scale())
            out.append({"guard": opt.guard_dev.clone(), "p": opt.flat_p.clone(), "m": opt.exp_avg.clone(), "g": opt.flat_g.clone()})
        ret[rank] = {"steps": out, "own": own, "segs": [opt.segment(i) for i in range(4)], "step": float(opt.step_dev)}
    dist.destroy_process_group()


def test_two_ranks_take_the_same_decisions():
    world, port = 2, _free_port()
    ret = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, ret), nprocs=world, join=True)
    r0, r1 = ret[0], ret[1]
    for a, b in zip(r0["steps"], r1["steps"]):
        for k in ("guard", "p", "m", "g"):
            assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), k           # (bits: a skipped row's norm is NaN)
    assert r0["own"] != r1["own"] and r0["step"] == 3.0
    s0, s1, s2 = r0["steps"]
    # the norm is that of the MEAN gradient (what Adam consumes): 0.5 * ||sum||
    for i, (lo, hi) in enumerate(r0["segs"]):
        want = 0.5 * float(s0["g"][lo:hi].double().norm())
        assert abs(float(s0["guard"][i, 0]) - want) < 1e-6 * want
    assert s0["guard"][:, 1:4].tolist() == [[1.0, 1.0, 0.0]] * 4
    # one rank's NaN: PoseNet skipped on both, the others updated
    lo, hi = r0["segs"][1]
    assert s1["guard"][:, 2].tolist() == [1.0, 0.0, 1.0, 1.0] and s1["guard"][:, 3].tolist() == [0.0, 1.0, 0.0, 0.0]
    assert torch.equal(s1["p"][lo:hi], s0["p"][lo:hi]) and torch.equal(s1["m"][lo:hi], s0["m"][lo:hi])
    assert not torch.equal(s1["p"][:lo], s0["p"][:lo]) and bool(torch.isfinite(s1["p"]).all())
    # clipping from the value both ranks read
    assert 0.0 < float(s2["guard"][0, 1]) < 1.0 and s2["guard"][1:, 1].tolist() == [1.0] * 3
    assert s2["guard"][:, 3].tolist() == [0.0, 1.0, 0.0, 0.0]
