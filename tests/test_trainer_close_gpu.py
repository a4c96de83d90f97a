"""The end of a trainer's life on the MI355X: CCTrainer.close() gives the networks back as it found them."""
import pytest
import torch

from cc_amd import synthetic as syn, trainer as T

pytestmark = pytest.mark.gpu


def test_closed_trainer_leaves_its_networks_as_good_as_new():
    """CCTrainer.close() at 2 x 64 x 128, four networks, captured: the networks of a closed trainer, given back the seeded weights
    and buffers, carry a second trainer whose first step equals -- losses, parameter and gradient bucket, bit for bit (deterministic
    mode is the default) -- the first step of a trainer over freshly constructed networks.  The closed trainer refuses to step;
    closing it again does nothing."""
    dev = torch.device("cuda")
    bc = syn.sample(2, 64, 128, seed=1)
    batch = (bc[0].to(dev), [r.to(dev) for r in bc[1]], bc[2].to(dev), bc[3].to(dev))

    def seeded():
        nets = T.build_nets(dev, init=False)
        for n in nets:
            n.load_state_dict(syn.seeded_state_dict(n, 0))
        return nets

    def first_step(nets):
        tr = T.CCTrainer(nets, T.StepConfig(), use_graph=True)
        losses = {k: v.clone() for k, v in tr.step(batch).items()}
        assert tr.graph is not None
        return tr, (losses, tr.opt.flat_p.clone(), tr.opt.flat_g.clone())

    nets = seeded()
    saved = [{k: v.detach().clone() for k, v in n.state_dict().items()} for n in nets]
    tr, _ = first_step(nets)
    tr.step(batch)
    tr.close()
    assert tr.graph is None and tr.graph_b is None and tr.static_batch is None and tr.losses is None and tr.opt.sinks == {}
    lo, hi = tr.opt.flat_p.data_ptr(), tr.opt.flat_p.data_ptr() + 4 * tr.opt.flat_p.numel()
    assert not any(lo <= p.data_ptr() < hi or p.grad is not None for n in nets for p in n.parameters())
    with pytest.raises(RuntimeError, match="closed"):
        tr.step(batch)
    tr.close()
    for n, sd in zip(nets, saved):
        n.load_state_dict(sd)
    tr2, got = first_step(nets)
    tr3, want = first_step(seeded())
    assert sorted(got[0]) == sorted(want[0]) and all(torch.equal(got[0][k], want[0][k]) for k in want[0])
    assert torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])
    assert not torch.equal(got[1], tr.opt.flat_p)       # (two steps ahead: the closed trainer's bucket is nobody's weights)
    tr2.close()
    tr3.close()
