"""GPU: validation during training (run.py --valid_data_dir / --valid_steps).  Two short file-fed runs of run.py in child
processes on the shards of tests/filefed_data.py, one with validation and one without: the validated run trains the same bits,
only it records `valid` and writes best.pt, and what it records is what `--mode test --device_metrics True` computes from the
weights it saved - bit for bit, at the same batch size."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filefed_data as F                                         # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-newsrec_amd")
MODEL = ["--batch_size", "4", "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2", "--bert_trainable_layer",
         "0", "1", "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML", "--model_type", "tnlrv3",
         "--enable_hvd", "False", "--log_steps", "1"]
KEYS = ("auc", "mrr", "ndcg5", "ndcg10")


def _valid_set(dirname, n=11, seed=4):
    """news.tsv and one behaviours file in test format: `iid uid time history N1-0 N2-1 ...`; impressions of 1 to 12
    candidates, one without a positive, one without a negative, one with a single candidate, an unknown id among them."""
    rs = np.random.RandomState(seed)
    ids = F.news_ids()
    os.makedirs(dirname)
    with open(F.NEWS) as src, open(os.path.join(dirname, "news.tsv"), "w") as out:
        out.write(src.read())
    with open(os.path.join(dirname, "behaviors_0.tsv"), "w") as f:
        for j in range(n):
            hist = [ids[k] for k in rs.randint(0, len(ids), int(rs.randint(0, 60)))]
            C = 1 if j == 5 else int(rs.randint(2, 13))
            labs = rs.randint(0, 2, C)
            if j == 2:
                labs[:] = 0
            if j == 7:
                labs[:] = 1
            if j not in (2, 5, 7):
                labs[0], labs[1] = 1, 0
            cand = [ids[k] for k in rs.randint(0, len(ids), C)]
            if j == 3:
                cand[0] = F.UNKNOWN
            f.write("%d\tU%d\t11/15/2019 8:55:22 AM\t%s\t%s\n" % (j, j, " ".join(hist), " ".join("%s-%d" % (c, l) for c, l in zip(cand, labs))))
    return n


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    base = tmp_path_factory.mktemp("valid_in_train")
    d = str(base / "inputs")
    os.makedirs(d)
    F.make_shards(d + "/data", F.LINE_COUNTS, seed=0)
    embs, ckpts, tok = F.run_py_inputs(d)
    n_valid = _valid_set(d + "/valid")
    model = MODEL + tok
    train = ["--mode", "train", "--train_data_dir", d + "/data", "--filename_pat", "behaviors_np4_*.tsv", "--epochs", "1",
             "--max_steps_per_epoch", "3"] + model + ["--teacher_emb_paths"] + embs + ["--teacher_ckpts"] + ckpts
    env = dict(os.environ, PYTHONPATH=PKG)
    logs = {}
    for name, extra in (("plain", []), ("valid", ["--valid_data_dir", d + "/valid", "--valid_steps", "2"])):
        r = subprocess.run([sys.executable, "-u", os.path.join(PKG, "run.py")] + train + extra + ["--model_dir", str(base / name)],
                           env=env, capture_output=True, text=True, timeout=600, cwd=PKG)
        assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
        logs[name] = r.stdout + r.stderr
    return dict(base=base, valid_dir=d + "/valid", model=model, logs=logs, n_valid=n_valid)


def _load(p):
    return torch.load(str(p), map_location="cpu")


def test_a_validated_run_trains_the_same_bits(runs):
    plain, valid = _load(runs["base"] / "plain" / "epoch-1.pt"), _load(runs["base"] / "valid" / "epoch-1.pt")
    assert "valid" not in plain and list(plain) == ["model_state_dict", "category_dict", "word_dict", "subcategory_dict"]
    assert sorted(os.listdir(str(runs["base"] / "plain"))) == ["epoch-1.pt"]
    assert list(valid) == list(plain) + ["valid"]
    assert list(plain["model_state_dict"]) == list(valid["model_state_dict"])
    for k, v in plain["model_state_dict"].items():
        assert torch.equal(v, valid["model_state_dict"][k]), k
    assert "Valid:" not in runs["logs"]["plain"]
    # four batches (0 .. max_steps_per_epoch): validated behind batches 2 and 4; the epoch's end takes the second again
    assert runs["logs"]["valid"].count("] Valid: epoch 1 batch") == 2
    v = valid["valid"]
    assert sorted(v) == sorted(KEYS + ("seen", "scored", "epoch", "batch", "updates"))
    assert v["seen"] == runs["n_valid"] and v["scored"] == runs["n_valid"] - 3 and v["epoch"] == 1 and v["batch"] == 4
    assert 1 <= v["updates"] <= 4 and all(0.0 <= v[k] <= 1.0 for k in KEYS) and v["mrr"] > 0


@pytest.mark.parametrize("name", ["best.pt", "epoch-1.pt"])
def test_recorded_metrics_are_test_modes(runs, name):
    import parameters
    import run
    ck = _load(runs["base"] / "valid" / name)
    assert "optimizer_state_dict" not in ck and "model_state_dict" in ck
    args = parameters.parse_args(["--mode", "test", "--device_metrics", "True", "--model_dir", str(runs["base"] / "valid"),
                                  "--load_ckpt_name", name, "--test_data_dir", runs["valid_dir"], "--filename_pat",
                                  "behaviors_*.tsv"] + runs["model"])
    sums, n_local, n_metric = run.test(args)
    v = ck["valid"]
    assert n_local == v["seen"] and n_metric == v["scored"]
    for k, s in zip(KEYS, sums):
        assert v[k] == s / n_local, (k, v[k], s / n_local)
    if name == "best.pt":
        last = _load(runs["base"] / "valid" / "epoch-1.pt")["valid"]
        assert v["auc"] >= last["auc"] and v["batch"] in (2, 4)
