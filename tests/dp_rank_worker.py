"""One rank of tests/test_gpu_dp.py's two-rank run: `python dp_rank_worker.py RANK WORLD PORT OUT.npz`.

Both ranks share GPU 0 and rendezvous over gloo.  Each runs two data-parallel E updates (train_gen_recon.py:233-241) on
its shard of a B = 8 batch (8 positive and 16 negative latents) through damc.dist.sharded_step with verify=True, and
writes its pre-reduce bucket, its reduced bucket (both per update) and its final parameters to OUT."""
import datetime
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "diffusion-amortized-mcmc_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

B, NZ, MAX_NORM = 8, 128, 1.0


def main():
    rank, world, port, out = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3], sys.argv[4]
    import numpy as np
    import torch
    import torch.distributed as d

    from damc import dist, optim, synth
    from src import diffusion_net as dn

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=port)
    d.init_process_group("gloo", rank=rank, world_size=world, timeout=datetime.timedelta(seconds=90))
    dev = torch.device("cuda:0")
    E = synth.load_into(dn._netE(nz=NZ), 10).to(dev).train()
    opt = optim.Adam(E.parameters(), lr=2e-4, betas=(0.5, 0.999))
    zp = torch.from_numpy(synth.normal_f32(91, 0, (B, NZ))).to(dev)
    zn = torch.from_numpy(synth.normal_f32(91, 1, (2 * B, NZ))).to(dev)
    assert world == 2
    ps, pc = ((0, 3), (3, 5))[rank]  # 3 + 5 of B = 8: unequal shards, so the two scales differ
    before, after, norms = [], [], []
    reduce_ = dist.GradBucket.all_reduce

    def logged(self, group=None):
        before.append(self.buffer.detach().cpu().numpy().copy())
        r = reduce_(self, group)
        torch.cuda.synchronize()
        after.append(self.buffer.detach().cpu().numpy().copy())
        return r

    dist.GradBucket.all_reduce = logged
    for _ in range(2):
        opt.zero_grad()
        e_pos, e_neg = E(zp[ps:ps + pc]), E(zn[2 * ps:2 * (ps + pc)])
        (e_pos.mean() - e_neg.mean()).backward()
        norms.append(float(dist.sharded_step(opt, pc, B, max_norm=MAX_NORM, verify=True)))
    torch.cuda.synchronize()
    np.savez(out, norms=np.array(norms, dtype=np.float64), count=pc,
             **{"before%d" % i: a for i, a in enumerate(before)}, **{"after%d" % i: a for i, a in enumerate(after)},
             **{"param%d" % i: p.detach().cpu().numpy() for i, p in enumerate(E.parameters())})
    d.destroy_process_group()


if __name__ == "__main__":
    main()
