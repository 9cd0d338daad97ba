"""kpt_w_spectral on two gloo ranks (checker backend): the fit is replicated and the q list is sharded, so every rank packs its
own X and no new communication exists - K on two ranks must equal K on one rank (pattern of tests/test_multirank_cpu.py)."""
import os
import sys
import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

HERE = os.path.dirname(os.path.abspath(__file__))


def _setup_path():
    for p in (os.path.dirname(HERE), HERE):
        if p not in sys.path:
            sys.path.insert(0, p)


def _run_kcase(comm):
    _setup_path()
    import cells
    from kspectral_backend import KSpectralOracleBackend
    from pyscf_isdf_amd.isdf import ISDF
    cell = cells.cell_he2_triclinic()
    cell.mesh = np.array([8, 10, 9])
    kpts = cell.make_kpts([2, 2, 1])
    nao = cell.nao_nr()
    rng = np.random.default_rng(2)
    c = rng.standard_normal((4, nao, nao)) + 1j * rng.standard_normal((4, nao, nao))
    dms = np.einsum('kpi,kqi->kpq', c[:, :, :2], c[:, :, :2].conj())
    out = []
    for sphere in (0, 100):                      # whole box (twins from their own tables) and a sphere (conjugate twins)
        df = ISDF(cell, kpts=kpts, c_isdf=4, select='refined', backend=KSpectralOracleBackend(), comm=comm)
        df.kpt_w_spectral = True
        df.w_sphere = sphere
        vk = df.get_jk(dms, kpts=kpts, with_j=False)[1]
        assert df.w_spectral_fraction is not None
        out.append((df.ip.copy(), vk))
    return out


def _kworker(rank, world, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world),
                      LOCAL_RANK=str(rank))
    dist.init_process_group('gloo', rank=rank, world_size=world)
    _setup_path()
    from pyscf_isdf_amd.parallel import Comm
    out = _run_kcase(Comm.from_env())
    if rank == 0:
        q.put(out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_kpoints_spectral_two_ranks_match_one_rank():
    _setup_path()
    from pyscf_isdf_amd.parallel import Comm
    one = _run_kcase(Comm())
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 33500 + os.getpid() % 2000
    procs = [ctx.Process(target=_kworker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    two = q.get(timeout=240)
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    for (ip1, vk1), (ip2, vk2) in zip(one, two):
        assert np.array_equal(ip1, ip2)
        assert abs(vk1 - vk2).max() <= 1e-12 * abs(vk1).max()
