"""CPU: the host side of anomaly scoring (damc.anomaly, damc.dist.sharded_pr_auc, the two C entry points' argument
checks) and the anomaly golden against the fp32 oracle.  No device is touched."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch

from anomaly_util import RR_CHUNK, build_anomaly_case, host_generator_desc
from conftest import rel_l2

torch.set_num_threads(8)

# expected values: sklearn 1.7.2, auc(recall, precision) of precision_recall_curve(labels, scores)
PR_CASES = [
    ([0, 0, 1, 1], [0.1, 0.4, 0.35, 0.8], 0.7916666666666666),
    ([0, 1, 1, 0, 1, 0, 0, 1], [0.5, 0.5, 0.9, 0.2, 0.2, 0.2, 0.7, 0.9], 0.7958333333333334),  # ties across classes
    ([1, 1, 0, 0], [0.1, 0.2, 0.3, 0.4], 0.29166666666666663),
]


@pytest.mark.parametrize("labels,scores,want", PR_CASES)
def test_pr_auc_fixed_cases(labels, scores, want):
    from damc import anomaly

    got = anomaly.pr_auc(labels, scores)
    print("pr_auc", got, "expected", want)
    assert abs(got - want) <= 1e-12
    assert abs(anomaly.pr_auc(np.asarray(labels, dtype=bool), np.asarray(scores, dtype=np.float32).astype(np.float64))
               - want) <= 1e-12


def test_pr_auc_matches_sklearn_on_random_ties():
    metrics = pytest.importorskip("sklearn.metrics")
    from damc import anomaly

    rng = np.random.RandomState(0)
    worst = 0.0
    for _ in range(200):
        n = int(rng.randint(2, 60))
        y = rng.randint(0, 2, n)
        y[rng.randint(n)] = 1
        s = np.round(rng.rand(n), 2)  # two decimals: ties, within and across the classes
        p, r, _ = metrics.precision_recall_curve(y, s)
        worst = max(worst, abs(anomaly.pr_auc(y, s) - metrics.auc(r, p)))
    print("largest |pr_auc - sklearn| over 200 cases", worst)
    assert worst <= 1e-12


def test_pr_auc_rejects_bad_input():
    from damc import anomaly

    with pytest.raises(ValueError):
        anomaly.pr_auc([0, 1, 1], [0.1, np.nan, 0.3])
    with pytest.raises(ValueError):
        anomaly.pr_auc([0, 1, 1], [0.1, np.inf, 0.3])
    with pytest.raises(ValueError):
        anomaly.pr_auc([0, 1, 1], [0.1, 0.2])
    with pytest.raises(ValueError):
        anomaly.pr_auc([0, 0, 0], [0.1, 0.2, 0.3])


def test_module_does_not_import_sklearn():
    import ast

    from conftest import PKG

    for name in ("anomaly.py", "dist.py"):
        tree = ast.parse(open(os.path.join(PKG, "damc", name)).read())
        mods = [a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names]
        mods += [n.module or "" for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)]
        assert not [m for m in mods if m.split(".")[0] == "sklearn"], name


def test_energy_entry_points_host_only():
    """Size queries and argument checks of damc_recon_rows / damc_posterior_energy run on the host, before any launch
    (the pointers below are arbitrary non-null addresses that are never dereferenced)."""
    from damc import _lib
    from src import diffusion_net as dn

    L = _lib.lib()
    assert L.damc_abi_version() == 3
    ERR = _lib.DAMC_ERR_ARG
    q = L.damc_recon_rows_workspace_bytes
    assert q(1, 2) > 0
    assert q(21, 784) > q(1, 784)
    assert q(3, 2 * RR_CHUNK) < q(3, 2 * RR_CHUNK + 1) == q(3, 3 * RR_CHUNK)
    assert q(3, RR_CHUNK) == q(3, 784)  # one chunk either way
    assert q(0, 784) == 0 and q(-1, 784) == 0 and q(4, 0) == 0 and q(4, -5) == 0
    need = q(21, 784)
    ok = (256, 256, 21, 784, 256, 256, need, None)

    def rows(**kw):
        names = ("xhat", "x", "batch", "n", "out", "ws", "nbytes", "stream")
        a = dict(zip(names, ok))
        a.update(kw)
        return L.damc_recon_rows(*[a[k] for k in names])

    assert rows(out=None) == ERR and rows(xhat=None) == ERR and rows(x=None) == ERR
    assert rows(batch=0) == ERR and rows(batch=-3) == ERR
    assert rows(n=0) == ERR and rows(n=-784) == ERR
    assert rows(nbytes=need - 1) == ERR and rows(ws=None) == ERR  # a short workspace is an error, not an overrun

    g = host_generator_desc(dn._netG_mnist(nz=8, ngf=16, nc=1))
    pq = L.damc_posterior_energy_workspace_bytes
    n8, n21 = pq(ctypes.byref(g), 8), pq(ctypes.byref(g), 21)
    assert 0 < n8 < n21
    assert n21 > L.damc_posterior_workspace_bytes(ctypes.byref(g), 21) + 4 * 21 * 784  # the forward's own, and x_hat
    assert pq(ctypes.byref(g), 0) == 0 and pq(ctypes.byref(_lib.Generator()), 8) == 0 and pq(None, 8) == 0
    g_big = host_generator_desc(dn._netG_mnist(nz=8, ngf=32, nc=1))
    assert pq(ctypes.byref(g_big), 21) > n21
    e = _lib.Ebm()
    e.nz, e.nh, e.slope = 8, 200, 0.2
    okp = (ctypes.byref(g), ctypes.byref(e), 256, 256, 21, 1.0, 256, 256, None, 256, n21, None)

    def energy(**kw):
        names = ("g", "ebm", "z", "x", "batch", "rw", "terms", "score", "xhat", "ws", "nbytes", "stream")
        a = dict(zip(names, okp))
        a.update(kw)
        return L.damc_posterior_energy(*[a[k] for k in names])

    assert energy(terms=None) == ERR and energy(z=None) == ERR and energy(x=None) == ERR and energy(g=None) == ERR
    assert energy(batch=0) == ERR and energy(batch=-1) == ERR
    assert energy(nbytes=n21 - 1) == ERR and energy(ws=None) == ERR
    assert energy(g=ctypes.byref(_lib.Generator())) == ERR  # row_elems <= 0: an empty descriptor
    e.nz = 16
    assert energy() == ERR  # an EBM of another latent size


def test_oracle_reproduces_the_anomaly_golden():
    """The fixture is what it claims to be: the fp32 oracle, run from the golden's z0 on the drop-in nets, reproduces
    the reference's zK and score within the distances tests/test_oracle_golden.py allows (10 noiseless posterior
    steps: rel-L2 2e-4; E and G(z) at a given z: 1e-6; recon: 1e-5), and the record is self-consistent."""
    from oracle import damc_oracle as orc

    c = build_anomaly_case()
    rec, m = c["rec"], c["meta"]
    for key, mod in (("g_keys", c["G"]), ("e_keys", c["E"]), ("q_keys", c["Q"])):
        assert [[k, list(v.shape)] for k, v in mod.state_dict().items()] == m[key]
    assert rec["z0"].shape == rec["zK"].shape == (m["B"], m["nz"]) and rec["terms"].shape == (m["B"], 3)
    assert (m["steps"], m["step"], m["sigma"], m["recon_weight"]) == (5, 0.1, 1.0, 1.0)
    Lg, P = orc.generator_layers(c["G"]), orc.ebm_params(c["E"])
    z0, zK = torch.from_numpy(rec["z0"]), torch.from_numpy(rec["zK"])
    # the terms at the golden's own zK
    xh = orc.generator_sample(Lg, zK)
    recon = ((xh - c["x"]) ** 2).sum(dim=(1, 2, 3)).numpy()
    e = orc.ebm_energy_grad(P, zK)[0].numpy()
    hz = (0.5 * (zK ** 2).sum(1)).numpy()
    print("terms at golden zK: recon %.3e E %.3e z2 %.3e" % (
        np.max(np.abs(recon - rec["terms"][:, 0]) / rec["terms"][:, 0]), rel_l2(e, rec["terms"][:, 1]),
        rel_l2(hz, rec["terms"][:, 2])))
    assert np.max(np.abs(recon - rec["terms"][:, 0]) / rec["terms"][:, 0]) < 1e-5
    assert rel_l2(e, rec["terms"][:, 1]) < 1e-6
    assert rel_l2(hz, rec["terms"][:, 2]) < 1e-6
    assert np.array_equal(rec["score"], rec["terms"][:, 0] * np.float32(1) + rec["terms"][:, 1] + rec["terms"][:, 2])
    # the chain, then the score at the oracle's own end point
    zo = orc.posterior_langevin(Lg, P, z0, c["x"], m["steps"], m["sigma"], m["step"])
    so = (((orc.generator_sample(Lg, zo) - c["x"]) ** 2).sum(dim=(1, 2, 3)) + orc.ebm_energy_grad(P, zo)[0]
          + 0.5 * (zo ** 2).sum(1)).numpy()
    print("oracle chain: zK rel-L2 %.3e score rel-L2 %.3e" % (rel_l2(zo.numpy(), rec["zK"]), rel_l2(so, rec["score"])))
    assert rel_l2(zo.numpy(), rec["zK"]) < 2e-4
    assert rel_l2(so, rec["score"]) < 2e-4
    # z0 is Q(x): the chain has moved it, and it is finite
    assert np.all(np.isfinite(rec["z0"])) and rel_l2(rec["zK"], rec["z0"]) > 1e-3


# ------------------------------------------------------------------------------ sharded_pr_auc's gather, gloo world 2
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _StubQ:
    nz, with_noise = 4, True


def _stub_batches():
    # two global batches, ragged over 2 ranks: 21 = 11 + 10 and 5 = 3 + 2
    g = torch.Generator().manual_seed(3)
    return [torch.rand(21, 6, generator=g), torch.rand(5, 6, generator=g)]


def _stub_labels():
    return [(torch.arange(21) % 3 == 0).long(), torch.tensor([0, 1, 0, 0, 1])]


def _stub_scorer(log):
    def scorer(xs, zt, seed, chain_base):
        # a function of the row's data, its global draw and the global key alone, as the real scorer's is
        log.append((int(chain_base), int(xs.shape[0]), int(seed)))
        return xs.sum(1) + zt.sum(1) + float(seed % 7)
    return scorer


def _gather_worker(rank, world, port, q):
    import torch.distributed as d

    from damc import dist as ddist

    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    d.init_process_group("gloo", rank=rank, world_size=world)
    torch.manual_seed(11)
    log = []
    auc = ddist.sharded_pr_auc(_StubQ(), None, None, _stub_batches(), _stub_labels(), scorer=_stub_scorer(log))
    # the gather on its own: rank r's values are its global indices, so the result must be 0 .. 25
    parts = []
    for n, off in ((21, 0), (5, 21)):
        s, c = ddist.shard(n, rank, world)
        parts.append(torch.arange(s, s + c) + off)
    order = ddist.all_gather_shards(torch.cat(parts).float(), [21, 5]).numpy().copy()
    q.put((rank, auc, log, order))
    d.destroy_process_group()


def test_sharded_pr_auc_gathers_in_global_order():
    import torch.multiprocessing as mp

    from damc import anomaly
    from damc import dist as ddist

    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_gather_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    res = sorted(q.get(timeout=120) for _ in range(world))
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    # the single-process run of the same stub (world 1: no process group), and pr_auc of its scores directly
    torch.manual_seed(11)
    log1 = []
    want = ddist.sharded_pr_auc(_StubQ(), None, None, _stub_batches(), _stub_labels(), scorer=_stub_scorer(log1))
    torch.manual_seed(11)
    scores = []
    for x in _stub_batches():
        zt = torch.randn(x.shape[0], _StubQ.nz)
        seed = int(torch.randint(0, 2 ** 62, (1,), dtype=torch.int64).item())
        scores.append(_stub_scorer([])(x, zt, seed, 0))
    direct = anomaly.pr_auc(torch.cat(_stub_labels()).numpy(), torch.cat(scores).numpy())
    assert want == direct
    assert [(b, c) for b, c, _ in log1] == [(0, 21), (0, 5)]
    for rank, auc, log, order in res:
        assert auc == want, (rank, auc, want)
        assert np.array_equal(order, np.arange(26, dtype=np.float64)), order  # ragged shards unpadded, global order
        assert [(b, c) for b, c, _ in log] == ([(0, 11), (0, 3)] if rank == 0 else [(11, 10), (3, 2)])
        assert [s for _, _, s in log] == [s for _, _, s in log1]  # the same global key on every rank
