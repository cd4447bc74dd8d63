"""distributed.all_reduce_image on CPU (world_size-2 gloo group): the images of the shards of a row set, binned on one shared window, add
to the image of the whole set exactly.  The binning here is the numpy rule; the engine's is held to it in test_spot_readout.py."""
import os
import socket
import sys

import numpy as np
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import spot_ref as sr
    from bmo_amd import distributed as bd

    window = (-1e-3, 1e-3, -2e-3, 1e-3)
    rows = sr.window_rows(3001, window, seed=4)
    lo, hi = bd.shard_bounds(len(rows), rank, world)
    mine, _ = sr.bin_rule(rows[lo:hi], window, 40, 24)
    total = bd.all_reduce_image(torch.from_numpy(mine.copy())).numpy()
    whole, _ = sr.bin_rule(rows, window, 40, 24)
    assert total.dtype == np.int64 and np.array_equal(total, whole) and whole.sum() > 1000
    try:
        bd.all_reduce_image(torch.zeros(4, dtype=torch.float64))
        refused = False
    except TypeError:
        refused = True
    assert refused
    open(os.path.join(out_dir, "ok%d" % rank), "w").write("ok")
    dist.barrier()
    dist.destroy_process_group()


def test_shard_images_add_exactly(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    assert (tmp_path / "ok0").exists() and (tmp_path / "ok1").exists()
