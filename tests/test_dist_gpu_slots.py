"""Multi-process rehearsal of the gather_kind "slots" gather on ONE GPU: world_size
2 and 3, every rank on cuda:0, gloo for the exchange (as test_dist_gpu.py's stream
gather).  `world` images are encoded as row shards and gathered in one grouped
batch (image j to rank j, sharding.gather_streams_group): the ranks ship their
blocks in the wire format, the receiving rank fills its slot landing zone from the
segments and its own blocks and closes it.  Each rank's received image must equal
its single-GPU encode bit for bit, and be None elsewhere."""
import os
import tempfile

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from test_dist_gpu import _free_port, _image

pytestmark = pytest.mark.gpu


def _rank(rank, world, port, H, W, out_path):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY="0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from hiccup_amd import device, pipeline, sharding
    torch.cuda.set_device(0)
    rgb = _image(H, W)
    s = torch.cuda.Stream()  # a non-current stream: the gather and the fill must follow it
    xgroup = dist.new_group(list(range(world)))
    imgs = [np.roll(rgb, 8 * j, axis=1) for j in range(world)]
    ses = [sharding.ShardEncoder(H, W, rank=rank, world=world, gather_to=j, gather_kind="slots")
           for j in range(world)]
    a, b = ses[0].span
    ok = True
    for _ in range(2):  # the second round reuses the cached job arrays and buffers
        sharding.encode_group(ses, [device.to_device(img[a:b]) for img in imgs], stream=s)
        wholes = sharding.gather_streams_group(ses, group=xgroup, stream=s)
        torch.cuda.synchronize()
        ref_enc = pipeline.Encoder(H, W)
        ref_enc.encode(device.to_device(imgs[rank]))
        ref = ref_enc.result()
        mine = wholes[rank]
        ok &= mine is ses[rank].whole and mine.slots and isinstance(mine.index, pipeline.SlotIndex)
        got = mine.result()
        ok &= all(np.array_equal(got[k][i], ref[k][i]) for k in pipeline.CHANNELS for i in range(4))
        ok &= all(wholes[j] is None for j in range(world) if j != rank)
        ok &= all(int(e.wire_flag.item()) == 0 for e in ses)
    oks = [None] * world
    dist.all_gather_object(oks, bool(ok))
    if rank == 0:
        with open(out_path, "w") as f:
            f.write("ok" if all(oks) else "mismatch %s" % oks)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,H,W", [(2, 256, 1024), (3, 96, 512)])
def test_slots_gather_multiprocess(world, H, W):
    with tempfile.TemporaryDirectory() as d:
        out = os.path.join(d, "result")
        mp.spawn(_rank, args=(world, _free_port(), H, W, out), nprocs=world, join=True)
        assert open(out).read() == "ok"
