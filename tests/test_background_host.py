"""Static background removal, the parts that need no GPU: the background= argument is checked in the constructor (an
empty folder, so no device is touched), and reduce_background makes the ranks agree on the elementwise minimum (two
gloo processes, as in test_dist_gloo.py)."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.multiprocessing as mp


def test_background_argument_is_checked_before_the_gpu(tmp_path):
    from torchpiv_amd import backend as T
    bad = [
        "mean",                                                        # unknown string
        np.zeros((8, 8), dtype=np.uint16),                             # wrong dtype (numpy)
        torch.zeros((8, 8), dtype=torch.float32),                      # wrong dtype (torch)
        np.zeros((2, 8, 8), dtype=np.uint8),                           # a stack is not an image
        np.zeros(8, dtype=np.uint8),                                   # nor is a row
        (np.zeros((8, 8), np.uint8), np.zeros((8, 9), np.uint8)),      # a pair of two shapes
        (np.zeros((8, 8), np.uint8),) * 3,                             # three images
        [[0, 1], [2, 3]],                                              # not an array
    ]
    for bg in bad:
        with pytest.raises(ValueError):
            T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, background=bg)
    for good in (None, "min", np.zeros((8, 8), np.uint8), torch.zeros((8, 8), dtype=torch.uint8),
                 (np.zeros((8, 8), np.uint8), torch.ones((8, 8), dtype=torch.uint8))):
        piv = T.OfflinePIV(str(tmp_path), "cpu", "bmp", 64, 32, background=good)
        assert len(piv) == 0 and list(piv()) == []
    # the runner passes the argument through (and its check)
    from torchpiv_amd import runner
    with pytest.raises(ValueError):
        runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, background="median")
    assert runner.run_folder(str(tmp_path), "cpu", "bmp", 64, 32, background="min") == (None, 0)


def test_background_argument_shape_against_the_frames(tmp_path):
    """A folder with frames: the images must have the frame shape (checked before the GPU check, which fails here on a
    machine without one -- that is the RuntimeError)."""
    from PIL import Image

    from torchpiv_amd import backend as T
    rng = np.random.default_rng(3)
    for k in range(2):
        for s in "ab":
            Image.fromarray(rng.integers(0, 256, (24, 40)).astype(np.uint8), "L").save(tmp_path / f"im{k}_{s}.bmp")
    with pytest.raises(ValueError):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 16, 8, background=np.zeros((40, 24), np.uint8))
    with pytest.raises(RuntimeError):
        T.OfflinePIV(str(tmp_path), "cpu", "bmp", 16, 8, background=np.zeros((24, 40), np.uint8))


def test_reduce_background_single_process_is_identity():
    from torchpiv_amd import dist as pdist
    a = torch.arange(12, dtype=torch.uint8).view(3, 4)
    assert pdist.reduce_background(a) is a
    pair = (a, a.flip(0))
    assert pdist.reduce_background(pair) is pair


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _images(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return (torch.randint(0, 256, (5, 7), generator=g, dtype=torch.uint8),
            torch.randint(0, 256, (5, 7), generator=g, dtype=torch.uint8))


def _worker(rank, world, port, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank),
                      WORLD_SIZE=str(world), LOCAL_RANK=str(rank))
    from torchpiv_amd import dist as pdist
    pdist.init_from_env(backend="gloo")
    bg_a, bg_b = _images(rank)
    ra, rb = pdist.reduce_background((bg_a, bg_b))
    single = pdist.reduce_background(bg_a.clone())
    q.put((rank, ra.numpy(), rb.numpy(), single.numpy(), str(ra.dtype), str(single.dtype)))
    # the inputs are left as they were
    assert torch.equal(bg_a, _images(rank)[0]) and torch.equal(bg_b, _images(rank)[1])
    import torch.distributed as dist
    dist.destroy_process_group()


def test_reduce_background_two_gloo_ranks():
    world, port = 2, _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for p in procs:
        p.start()
    got = [q.get(timeout=120) for _ in range(world)]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    want_a = np.minimum(_images(0)[0].numpy(), _images(1)[0].numpy())
    want_b = np.minimum(_images(0)[1].numpy(), _images(1)[1].numpy())
    assert not np.array_equal(want_a, _images(0)[0].numpy())         # the ranks really differ
    for rank, ra, rb, single, dt_pair, dt_single in got:
        assert dt_pair == dt_single == "torch.uint8"
        assert np.array_equal(ra, want_a) and np.array_equal(rb, want_b), rank
        assert np.array_equal(single, want_a), rank
