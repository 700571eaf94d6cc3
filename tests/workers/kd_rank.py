"""One rank of `post_train_kd.py` for tests/test_kd_files_gpu.py (started once per rank with RANK / WORLD_SIZE / LOCAL_RANK=0 /
MASTER_ADDR / MASTER_PORT in the environment, like tests/workers/run_rank.py).

    python kd_rank.py OUT_DIR <post_train_kd.py's flags>

The process group is initialised HERE, over gloo, before post_train_kd.train() is called: utils.init_hvd_cuda then finds a group
and keeps it, so both ranks share cuda:0 and dist.GradSync takes its host-staged path.  Nothing of the product is patched; train()
returns its engine.  Afterwards OUT_DIR/rank<r>.npz holds what the ranks must agree on - the trainable parameters, Adam's three
moment buffers, the update count, the loss scale and the skipped steps.  Exit status 1 on any exception."""
import os
import sys
import traceback

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tiny-newsrec_amd"))


def main(out_dir, argv):
    import dist as D
    import post_train_kd
    import utils
    utils.setuplogger()
    world, rank, _ = D.init("gloo")
    eng = post_train_kd.train(post_train_kd.parse_args(argv)).title
    torch.cuda.synchronize()
    host = lambda t: t.detach().cpu().numpy()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), params=host(eng.flat[True]), adam_m=host(eng.adam_m), adam_v=host(eng.adam_v),
             adam_vmax=host(eng.adam_vmax), step_count=np.int64(eng.step_count), gscale=np.float64(eng.gscale),
             skipped=np.int64(eng.scaler.skipped))
    D.barrier()
    if torch.distributed.is_initialized():
        torch.distributed.destroy_process_group()


if __name__ == "__main__":
    try:
        main(sys.argv[1], sys.argv[2:])
    except BaseException:          # noqa: BLE001 - the launcher reads the log and the exit status
        traceback.print_exc()
        sys.stdout.flush()
        sys.stderr.flush()
        os._exit(1)
