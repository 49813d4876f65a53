"""GPU: per-sample posterior energy (csrc/energy.hip: damc_recon_rows, damc_posterior_energy) and the anomaly scoring
calls built on it (damc.anomaly, damc.dist.sharded_pr_auc).

Tolerances.  damc_recon_rows against fp64: |out - ref| <= n 2^-23 sum (xhat - x)^2 per row, the worst-case bound of any
summation order of n fp32 terms.  damc_posterior_energy: the project's 3x rule -- over the batch vector
of the score and of each term, |hip - fp64| <= 3 |stock fp32 - fp64| in L2, where stock fp32 is the drivers' torch
expression on the stock modules on the GPU (or, for the golden case, the reference's recorded values).  Everything
about batch composition is bitwise."""
import copy
import functools

import numpy as np
import pytest
import torch

from anomaly_util import RR_CHUNK, build_anomaly_case, driver_terms, l2, oracle_terms
from conftest import SEED_QN, build_g_case

pytestmark = pytest.mark.gpu

ROW_SHAPES = [(1, 2), (21, 2),            # rows at 8-byte alignment: scalar loads
              (21, 784),                  # MNIST: one ragged chunk, 16-byte loads
              (5, 3072),
              (3, RR_CHUNK + 4), (3, 2 * RR_CHUNK),  # a 4-element last chunk; two full chunks
              (3, RR_CHUNK + 3),          # ragged quad in the last chunk, scalar loads across a chunk boundary
              (2, 196608)]                # CelebA-HQ 3 x 256 x 256: 12 chunks


@functools.lru_cache(maxsize=None)
def _row_inputs(shape):
    """(xhat, x) uniform in [-1, 1] (fp32, CPU) and the fp64 row sums; computed once, read-only."""
    g = torch.Generator().manual_seed(shape[0] * 1000003 + shape[1])
    xhat = torch.rand(*shape, generator=g) * 2 - 1
    x = torch.rand(*shape, generator=g) * 2 - 1
    ref = ((xhat.double() - x.double()) ** 2).sum(1).numpy()
    return xhat, x, ref


def _guarded(t, device, lead=0):
    """t as the leading part (after `lead` floats) of a larger device buffer whose remainder is NaN."""
    buf = torch.full((lead + t.numel() + 8192,), float("nan"), dtype=torch.float32, device=device)
    buf[lead:lead + t.numel()] = t.reshape(-1).to(device)
    return buf[lead:lead + t.numel()].view(t.shape)


@pytest.mark.parametrize("shape", ROW_SHAPES, ids=lambda s: "%dx%d" % s)
def test_recon_rows_vs_fp64(gpu_device, shape):
    """Every load path and chunk boundary against fp64, from inputs that end where NaN begins (no over-read), and from
    a base 4 bytes past a 16-byte boundary (the scalar-load instantiation), which gives the same bits."""
    from damc import anomaly

    xhat, x, ref = _row_inputs(shape)
    n = shape[1]
    out = anomaly.recon_rows(_guarded(xhat, gpu_device), _guarded(x, gpu_device)).cpu().numpy()
    assert np.all(np.isfinite(out))
    err, bound = np.abs(out.astype(np.float64) - ref), n * 2.0 ** -23 * ref
    print("recon_rows", shape, "max err / bound %.3e" % float(np.max(err / bound)))
    assert np.all(err <= bound)
    xs, xh = _guarded(x, gpu_device, lead=1), _guarded(xhat, gpu_device, lead=1)
    assert xs.data_ptr() % 16 == 4 and xs.is_contiguous()
    out_s = anomaly.recon_rows(xh, xs).cpu().numpy()
    assert np.array_equal(out_s, out)


@pytest.mark.parametrize("shape", [(21, 784), (3, 2 * RR_CHUNK)], ids=lambda s: "%dx%d" % s)
def test_recon_rows_do_not_depend_on_the_batch(gpu_device, shape):
    """A row's sum depends on that row's data and its length only: rows computed alone (from a pointer into the batch),
    in shards, and in a row-permuted batch equal the whole batch's bit for bit."""
    from damc import anomaly

    xhat, x, _ = _row_inputs(shape)
    xh, xd = _guarded(xhat, gpu_device), _guarded(x, gpu_device)
    B = shape[0]
    whole = anomaly.recon_rows(xh, xd)
    alone = torch.cat([anomaly.recon_rows(xh[i:i + 1], xd[i:i + 1]) for i in range(B)])
    assert torch.equal(alone, whole)
    cut = 5 if B > 5 else 1
    shards = torch.cat([anomaly.recon_rows(xh[:cut], xd[:cut]), anomaly.recon_rows(xh[cut:], xd[cut:])])
    assert torch.equal(shards, whole)
    perm = torch.randperm(B, generator=torch.Generator().manual_seed(1)).to(gpu_device)
    permuted = anomaly.recon_rows(_guarded(xh[perm], gpu_device), _guarded(xd[perm], gpu_device))
    assert torch.equal(permuted, whole[perm])
    assert torch.isfinite(whole).all()


# ----------------------------------------------------------------------------------- posterior_energy against fp64
def _case_golden():
    c = build_anomaly_case()
    z = torch.from_numpy(c["rec"]["zK"])
    return c["G"], c["E"], z, c["x"]


def _case_cifar():
    c = build_g_case("cifar10_w16")
    return c["G"], c["E"], c["z0"], c["x"]


def _case_toy():
    from damc import synth
    from damc.toy import ToyG

    G = synth.load_into(ToyG(), 0).eval()
    z = torch.from_numpy(synth.normal_f32(2, 0, (21, 2)))
    x = torch.from_numpy(synth.uniform_f32(1, 0, (21, 2)))
    return G, None, z, x


def _case_specnorm():
    """_netG_mnist(use_spc_norm=True) in eval mode, after two train-mode forwards so that u, v are power-iterated."""
    from damc import synth
    from src import diffusion_net as dn

    G = synth.load_into(dn._netG_mnist(nz=8, ngf=16, nc=1, use_spc_norm=True), 4)
    E = synth.load_into(dn._netE(nz=8), 10).eval()
    z = torch.from_numpy(synth.normal_f32(45, 0, (9, 8)))
    x = torch.from_numpy(synth.uniform_f32(45, 1, (9, 1, 28, 28)))
    G.train()
    with torch.no_grad():
        G(z), G(z)
    return G.eval(), E, z, x


ENERGY_CASES = {"golden": _case_golden, "cifar10_w16": _case_cifar, "toy": _case_toy, "specnorm": _case_specnorm}


def _truth(name, G, E, z, x, rw):
    """The terms in fp64 on CPU copies of the same nets: the oracle, or for the spectral-norm generator (whose weight
    is the hook's W / sigma) the stock modules cast to fp64."""
    if name == "specnorm":
        return driver_terms(copy.deepcopy(G).double(), copy.deepcopy(E).double(), z.double(), x.double(), rw)
    return oracle_terms(G, E, z, x, rw)


@pytest.mark.parametrize("name", sorted(ENERGY_CASES))
def test_posterior_energy_vs_fp64(gpu_device, name):
    from damc import anomaly, langevin, training

    G, E, z, x = ENERGY_CASES[name]()
    sigma = 0.3
    Gd, Ed = G.to(gpu_device), (E.to(gpu_device) if E is not None else None)
    zd, xd = z.to(gpu_device), x.to(gpu_device)
    z_keep, x_keep = zd.clone(), xd.clone()
    for rw in (1.0, 0.5 / sigma ** 2):
        t64, s64 = _truth(name, copy.deepcopy(G).cpu(), copy.deepcopy(E).cpu() if E is not None else None, z, x, rw)
        with training.stock_pytorch():
            t32, s32 = driver_terms(Gd, Ed, zd, xd, rw)
        terms, score, xhat = anomaly.posterior_energy(zd, xd, Gd, Ed, recon_weight=rw, return_xhat=True)
        terms2, score2 = anomaly.posterior_energy(zd, xd, Gd, Ed, recon_weight=rw)
        assert torch.equal(zd, z_keep) and torch.equal(xd, x_keep)  # read, never written
        assert torch.equal(terms, terms2) and torch.equal(score, score2)  # x_hat in the workspace or in the caller's
        assert torch.equal(xhat, langevin.generator_forward(zd, Gd))
        assert terms.shape == (len(z), 3) and score.shape == (len(z),)
        # the score is the expression on the fp32 terms, each operation rounded on its own
        again = torch.tensor(rw, dtype=torch.float32, device=gpu_device) * terms[:, 0] + terms[:, 1] + terms[:, 2]
        assert torch.equal(score, again)
        if E is None:
            assert torch.count_nonzero(terms[:, 1]) == 0
        th, sh = terms.cpu().numpy(), score.cpu().numpy()
        assert np.all(np.isfinite(th)) and np.all(np.isfinite(sh))
        pairs = [("score", sh, s32, s64)] + [("term%d" % k, th[:, k], t32[:, k], t64[:, k]) for k in range(3)]
        for what, h, r32, r64 in pairs:
            e_hip, e_ref = l2(h, r64), l2(r32, r64)
            print("%s rw=%.3g %s: |hip-fp64| %.3e  |stock fp32-fp64| %.3e  |fp64| %.3e"
                  % (name, rw, what, e_hip, e_ref, float(np.linalg.norm(r64))))
            assert e_hip <= 3 * e_ref, (name, rw, what, e_hip, e_ref)


def test_posterior_energy_rows_do_not_depend_on_the_batch(gpu_device):
    """Given identical z, the energy call's rows are bitwise the same alone, in shards and in the whole batch."""
    from damc import anomaly

    c = build_anomaly_case(gpu_device)
    z, x = torch.from_numpy(c["rec"]["zK"]).to(gpu_device), c["x"]
    tw, sw = anomaly.posterior_energy(z, x, c["G"], c["E"])
    for cuts in ([0, 5, 21], [0, 8, 16, 21], [0, 1, 2, 21]):
        for a, b in zip(cuts[:-1], cuts[1:]):
            t, s = anomaly.posterior_energy(z[a:b].contiguous(), x[a:b].contiguous(), c["G"], c["E"])
            assert torch.equal(t, tw[a:b]) and torch.equal(s, sw[a:b]), (a, b)


def test_posterior_energy_replays_from_a_captured_graph(gpu_device):
    """The call neither synchronises the host nor leaves the caller's stream: captured into a graph (as
    tests/test_gpu_graph.py captures the chains) and replayed on two inputs, it equals the eager call bitwise."""
    from damc import anomaly

    c = build_anomaly_case(gpu_device)
    G, E, x = c["G"], c["E"], c["x"]
    zs = [torch.from_numpy(c["rec"][k]).to(gpu_device) for k in ("zK", "z0")]
    eager = [anomaly.posterior_energy(z, x, G, E) for z in zs]
    torch.cuda.synchronize()
    zg = zs[0].clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        anomaly.posterior_energy(zg.clone(), x, G, E)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tg, sg = anomaly.posterior_energy(zg, x, G, E)
    for z, (te, se) in zip(zs, eager):
        zg.copy_(z)
        graph.replay()
        torch.cuda.synchronize()
        assert torch.equal(tg, te) and torch.equal(sg, se)


def test_golden_score(gpu_device):
    """From the reference's z0: 5 noiseless posterior steps, then the energy, against the reference's recorded zK-score
    by the 3x rule with the fp64 oracle chain (from the same z0) as the truth."""
    from damc import anomaly, langevin
    from oracle import damc_oracle as orc

    c = build_anomaly_case()
    rec, m = c["rec"], c["meta"]
    z0 = torch.from_numpy(rec["z0"])
    z64 = orc.posterior_langevin(orc.generator_layers(c["G"], torch.float64), orc.ebm_params(c["E"], torch.float64),
                                 z0.double(), c["x"].double(), m["steps"], m["sigma"], m["step"])
    t64, s64 = oracle_terms(c["G"], c["E"], z64, c["x"], m["recon_weight"])
    G, E, x = c["G"].to(gpu_device), c["E"].to(gpu_device), c["x"].to(gpu_device)
    z = z0.to(gpu_device).clone()
    langevin.posterior_langevin(z, x, G, E, m["steps"], m["sigma"], m["step"], False)
    terms, score = anomaly.posterior_energy(z, x, G, E, recon_weight=m["recon_weight"])
    th, sh = terms.cpu().numpy(), score.cpu().numpy()
    pairs = [("z", z.cpu().numpy(), rec["zK"], z64.numpy()), ("score", sh, rec["score"], s64)]
    pairs += [("term%d" % k, th[:, k], rec["terms"][:, k], t64[:, k]) for k in range(3)]
    for what, h, g, r64 in pairs:
        e_hip, e_ref = l2(h, r64), l2(g, r64)
        print("golden %s: |hip-fp64| %.3e  |golden-fp64| %.3e  |fp64| %.3e"
              % (what, e_hip, e_ref, float(np.linalg.norm(r64))))
        assert e_hip <= 3 * e_ref, (what, e_hip, e_ref)


# ------------------------------------------------------------------------------------------------ the one-call forms
@pytest.fixture(scope="module")
def scored(gpu_device):
    """The golden nets on the device, a fixed zt and sweep key, and anomaly.score of the whole batch."""
    from damc import anomaly, synth

    c = build_anomaly_case(gpu_device)
    B, nz = c["meta"]["B"], c["meta"]["nz"]
    zt = torch.from_numpy(synth.normal_f32(SEED_QN, 0, (B, nz)))
    seed = 0x5EED1234
    s, z = anomaly.score(c["Q"], c["G"], c["E"], c["x"], zt=zt, seed=seed)
    return dict(c=c, zt=zt, seed=seed, score=s, z=z)


def test_score_equals_its_parts(gpu_device, scored):
    from damc import amortizer, anomaly, langevin

    c, x = scored["c"], scored["c"]["x"]
    with torch.no_grad():
        z = amortizer.q_forward(c["Q"], x=x, zt=scored["zt"], seed=scored["seed"])
    langevin.posterior_langevin(z, x, c["G"], c["E"], 5, 1.0, 0.1, False)
    _, s = anomaly.posterior_energy(z, x, c["G"], c["E"])
    assert torch.equal(z, scored["z"]) and torch.equal(s, scored["score"])
    assert torch.isfinite(s).all() and s.shape == (c["meta"]["B"],)


@pytest.mark.parametrize("cuts", [[0, 5, 21], [0, 8, 16, 21]], ids=["5+16", "8+8+5"])
def test_score_shards_equal_the_whole_batch(gpu_device, scored, cuts):
    """Shards with chain_base = the slice start reproduce the whole batch's z and scores bit for bit."""
    from damc import anomaly

    c, x = scored["c"], scored["c"]["x"]
    for a, b in zip(cuts[:-1], cuts[1:]):
        s, z = anomaly.score(c["Q"], c["G"], c["E"], x[a:b].contiguous(), zt=scored["zt"][a:b], seed=scored["seed"],
                             chain_base=a)
        dz = int((z != scored["z"][a:b]).sum())
        print("shard [%d:%d): %d of %d z values differ from the whole batch's" % (a, b, dz, z.numel()))
        assert torch.equal(z, scored["z"][a:b]), (a, b)
        assert torch.equal(s, scored["score"][a:b]), (a, b)


def test_sharded_pr_auc_world_1(gpu_device, scored):
    """No process group: sharded_pr_auc equals pr_auc of anomaly.score over the same batches with the same draws."""
    from damc import anomaly
    from damc import dist as ddist

    c, x = scored["c"], scored["c"]["x"]
    batches = [x[:13], x[13:]]
    labels = (np.arange(21) % 4 == 1).astype(np.int64)
    torch.manual_seed(5)
    got = ddist.sharded_pr_auc(c["Q"], c["G"], c["E"], batches, labels)
    torch.manual_seed(5)
    scores = torch.cat([anomaly.score(c["Q"], c["G"], c["E"], xb)[0] for xb in batches])
    want = anomaly.pr_auc(labels, scores.cpu().numpy())
    assert got == want and 0.0 < got <= 1.0
    torch.manual_seed(5)  # labels given per batch
    assert got == ddist.sharded_pr_auc(c["Q"], c["G"], c["E"], batches, [labels[:13], labels[13:]])
