"""run.py --mode train as a real run goes through it: at two ranks, from files, and resumed.

Every launch is tests/workers/run_rank.py once per rank (gloo, both ranks on cuda:0 - the form tests/test_dp_gpu.py uses for the
engine), which calls run.train() and dumps what the ranks must agree on.  Each case is the A / B / C scheme of
tests/test_resume_gpu.py::test_run_py_resumes_bit_for_bit: A runs two epochs, B one epoch with --save_optimizer True, C
--resume True from B's epoch-1.pt up to epoch 2 in B's directory.  EVERY comparison is torch.equal / np.array_equal (that test's
_equal walker), except the one bounded gradient norm of test_scale_of_the_exchanged_gradient.

  synthetic, world 2   the ranks train on different impressions (synth.impressions(77 + rank)): equal buffers can only come from
                       the exchange (model._after_bucket = sync.launch, TnrAdam(model, ..., sync)); rank 1 of C gets its moments
                       through the resume path's dist.broadcast_flat; only rank 0 writes files.
  file-fed, world 1    the shards of tests/filefed_data.py through the three feed forms (--decode_process child, producer
                       thread, --resident_tables False): `loader.epoch = first_epoch - 1` and the label stream of a resumed
                       process; the forms agree with each other.
  file-fed, world 2    the per-epoch epoch_cap() (dist.min_over_ranks over shards that change every epoch: 6 steps, then 7) -
                       an uneven shard that is not capped deadlocks in the all-reduce, the launch's time limit would end it.

Launcher: at most two rank processes at a time (plus the loader's CPU-only decode child); both are polled, and when one exits
non-zero the other is killed at once instead of waiting inside a gloo collective; 300 s per launch guards against a hang; after
either nothing more is started by that test (a failed group of launches is remembered, not repeated).  Ports 29901 and up, one per
launch: 296xx belong to the other data-parallel tests, 297xx / 298xx to tests/test_host_cpu.py."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import filefed_data as F                                         # noqa: E402
from test_resume_gpu import _equal                               # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-newsrec_amd")
WORKER = os.path.join(ROOT, "tests", "workers", "run_rank.py")
LIMIT = 300.0                                                    # s per launch: a guard against hangs, not a measurement
_PORT = [29900]

MODEL = ["--mode", "train", "--batch_size", "4", "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2",
         "--bert_trainable_layer", "0", "1", "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML",
         "--model_type", "tnlrv3"]
ON = ["--warmup_steps", "3", "--lr_decay_steps", "40", "--weight_decay", "0.01", "--ema_decay", "0.9", "--max_grad_norm", "1",
      "--grad_accum_steps", "2"]
SYNTH = ["--synthetic", "True", "--max_steps_per_epoch", "6", "--log_steps", "1"]
FORMS = {"decode_process": [], "producer_thread": ["--decode_process", "False"], "rows_from_host": ["--resident_tables", "False"]}


class Launch:
    """What one launch left: logs[r] (stdout + stderr of rank r), npz[r] (its dump), dir (the --model_dir), seconds."""


def launch(out_dir, model_dir, flags, world):
    """run_rank.py once per rank with `flags` + --model_dir; fails the test (pytest.fail) on a non-zero exit or the time limit."""
    os.makedirs(out_dir, exist_ok=True)
    _PORT[0] += 1
    procs, files, t0 = [], [], time.time()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_PORT[0]))
        files.append(open(os.path.join(out_dir, "rank%d.log" % r), "w"))
        procs.append(subprocess.Popen([sys.executable, "-u", WORKER, out_dir] + flags + ["--model_dir", model_dir], env=env, cwd=PKG,
                                      stdout=files[-1], stderr=subprocess.STDOUT))
    tail = lambda r: open(os.path.join(out_dir, "rank%d.log" % r)).read()[-4000:]
    bad = None
    try:
        while bad is None and any(p.poll() is None for p in procs):
            for r, p in enumerate(procs):
                if p.poll() not in (None, 0):
                    bad = "rank %d of %s exited with status %s\n%s" % (r, out_dir, p.returncode, tail(r))
                    break
            else:
                if time.time() - t0 > LIMIT:
                    bad = "%s: no end after %.0f s\n%s" % (out_dir, LIMIT, "\n".join(tail(r) for r in range(world)))
                else:
                    time.sleep(0.02)
        for r, p in enumerate(procs):
            if bad is None and p.returncode != 0:
                bad = "rank %d of %s exited with status %s\n%s" % (r, out_dir, p.returncode, tail(r))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for f in files:
            f.close()
    if bad is not None:
        pytest.fail(bad, pytrace=False)
    res = Launch()
    res.logs = [open(os.path.join(out_dir, "rank%d.log" % r)).read() for r in range(world)]
    res.npz = [dict(np.load(os.path.join(out_dir, "rank%d.npz" % r))) for r in range(world)]
    res.dir, res.seconds = model_dir, time.time() - t0
    return res


def abc(root, flags, world, only_a=False):
    """-> {"A": Launch, "B": Launch, "C": Launch}"""
    root = str(root)
    save = ["--save_optimizer", "True"]
    out = {"A": launch(root + "/A.out", root + "/A", flags + save + ["--epochs", "2"], world)}
    if not only_a:
        out["B"] = launch(root + "/B.out", root + "/B", flags + save + ["--epochs", "1"], world)
        assert sorted(os.listdir(root + "/B")) == ["epoch-1.pt"]
        out["C"] = launch(root + "/C.out", root + "/B", flags + save + ["--epochs", "2", "--load_ckpt_name", "epoch-1.pt", "--resume", "True"],
                          world)
    print("\n%s: %s s" % (os.path.basename(root), " / ".join("%s %.1f" % (k, v.seconds) for k, v in out.items())))
    return out


_GROUPS = {}


def group(key, make):
    """A group of launches shared by several tests: made once, and a group that failed is not started again."""
    if key not in _GROUPS:
        try:
            _GROUPS[key] = make()
        except BaseException as e:          # noqa: BLE001 - pytest.fail raises one
            _GROUPS[key] = e
            raise
    if isinstance(_GROUPS[key], BaseException):
        pytest.fail("the launches of %s failed in an earlier test: %s" % (key, str(_GROUPS[key])[:2000]), pytrace=False)
    return _GROUPS[key]


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    return tmp_path_factory.mktemp("run_dp_resume")


@pytest.fixture(scope="module")
def filefed(base):
    """The shards, the tokenizer / config / teacher files, and run.py's flags for them."""
    d = str(base / "inputs")
    os.makedirs(d)
    F.make_shards(d + "/data", F.LINE_COUNTS, seed=0)
    embs, ckpts, tok = F.run_py_inputs(d)
    return MODEL + ON + ["--train_data_dir", d + "/data", "--filename_pat", "behaviors_np4_*.tsv"] + tok + \
        ["--teacher_emb_paths"] + embs + ["--teacher_ckpts"] + ckpts


def load(directory, name):
    return torch.load(os.path.join(directory, name), map_location="cpu")


def ranks_agree(run, what):
    a, b = run.npz
    assert sorted(a) == sorted(b), what
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "%s: rank 0 and rank 1 differ in %s" % (what, k)
    assert float(np.abs(a["adam_m"]).max()) > 0 and np.isfinite(a["params"]).all(), what


def c_equals_a(runs, updates, world, ema=True):
    """C's epoch-2.pt against A's; A's epoch-1.pt against B's; the counts."""
    a1, b1 = load(runs["A"].dir, "epoch-1.pt"), load(runs["B"].dir, "epoch-1.pt")
    a2, c2 = load(runs["A"].dir, "epoch-2.pt"), load(runs["C"].dir, "epoch-2.pt")
    keys = ["model_state_dict", "category_dict", "word_dict", "subcategory_dict"] + (["ema_state_dict", "ema"] if ema else []) + \
        ["optimizer_state_dict", "train_state"]
    assert list(a2) == list(c2) == keys
    for key in ("model_state_dict", "optimizer_state_dict") + (("ema_state_dict",) if ema else ()):
        _equal(a1[key], b1[key], "epoch 1 (A against B: fresh processes) " + key)
        _equal(a2[key], c2[key], key)
    _equal(a2["train_state"], c2["train_state"], "train_state")
    if ema:
        _equal(a2["ema"], c2["ema"], "ema")
    ts, osd = c2["train_state"], c2["optimizer_state_dict"]
    assert ts["epoch"] == 2 and ts["flags"]["world"] == world and ts["updates"] == osd["step"] and b1["train_state"]["epoch"] == 1
    skipped = osd["scaler"]["skipped"] if osd["scaler"] is not None else 0
    assert ts["updates"] + skipped == updates and ts["updates"] > b1["train_state"]["updates"] >= 1
    w = "student.news_encoder.dense.weight"
    assert not torch.equal(a2["model_state_dict"][w], a1["model_state_dict"][w])          # the second epoch did train
    return a2


def logs_of_a_resume(run):
    for r, log in enumerate(run.logs):
        assert "continuing at epoch 1" in log and "[%d] Resumed from" % r in log, log[-3000:]
        assert "the run that wrote" not in log, log[-3000:]


def only_rank_0_wrote(run, names, n_saved):
    assert sorted(os.listdir(run.dir)) == sorted(names)
    assert run.logs[0].count("Model saved to") == n_saved
    for log in run.logs[1:]:
        assert "Model saved to" not in log


# -- (a) synthetic, two ranks, fp16, everything on ---------------------------------------------------------------------------------
def synthetic_runs(base):
    return group("synthetic_w2", lambda: abc(base / "synthetic_w2", MODEL + ON + SYNTH, 2))


def test_synthetic_two_ranks_resume(base):
    runs = synthetic_runs(base)
    for k in "ABC":
        ranks_agree(runs[k], "synthetic, world 2, " + k)
        assert "ema" in runs[k].npz[0]
    # two epochs of 6 batches, windows of 2: three updates an epoch, unless fp16 skipped one
    c_equals_a(runs, 6, 2)
    a, c = runs["A"].npz[1], runs["C"].npz[1]
    assert sorted(a) == sorted(c)
    for k in a:          # rank 1 of C got its moments and the average through the broadcast, not from its own training
        assert np.array_equal(a[k], c[k]), "rank 1: C differs from A in " + k
    assert int(a["step_count"]) + int(a["skipped"]) == 6
    only_rank_0_wrote(runs["A"], ["epoch-1.pt", "epoch-2.pt"], 2)
    only_rank_0_wrote(runs["C"], ["epoch-1.pt", "epoch-2.pt"], 1)
    assert runs["B"].logs[0].count("Model saved to") == 1 and "Model saved to" not in runs["B"].logs[1]
    logs_of_a_resume(runs["C"])
    for log in runs["A"].logs:
        assert "world_size:2" in log


# -- (b) the reference's plain Adam / AMSGrad path under data parallelism ------------------------------------------------------------
def test_synthetic_two_ranks_bf16_all_options_off(base):
    run = abc(base / "synthetic_w2_bf16", MODEL + SYNTH + ["--dtype", "bf16"], 2, only_a=True)["A"]
    ranks_agree(run, "synthetic, world 2, bf16, options off")
    z = run.npz[0]
    assert "ema" not in z and int(z["step_count"]) == 12 and int(z["skipped"]) == 0          # an update per batch, no loss scaler
    only_rank_0_wrote(run, ["epoch-1.pt", "epoch-2.pt"], 2)
    assert load(run.dir, "epoch-2.pt")["train_state"]["flags"]["world"] == 2


# -- (e) the scale of the exchanged gradient -----------------------------------------------------------------------------------------
def test_scale_of_the_exchanged_gradient(base):
    """Adam normalises: a gradient that is summed instead of averaged over the ranks (x 2), or scaled by a wrong window length
    (x sqrt(2) .. 2), moves the parameters only slightly and identically on every rank.  run.py logs the clip's norm: with
    --grad_accum_steps 2 the first line that carries one is batch 1's, the norm of the first window's gradient averaged over
    2 ranks x 2 batches x 4 impressions.  Reference: ONE engine at world 1 with the same weights takes the same four batches as
    one window of four (Engine.backward(micro=(j, 4)), step(grad_scale=1 / 4) - the scale is stated here, not taken from
    TnrAdam or GradSync).  Bound: relative 1e-3, what tests/test_dp_gpu.py holds the two-rank-against-one-rank fp16 gradient
    itself to (the norm of a vector moves no more than the vector)."""
    import engine as E
    import hashinit
    import synth
    from dedup import build_plan
    from model_bert import engine_config_from_args
    from parameters import parse_args
    run = synthetic_runs(base)["A"]
    got = []
    for r, log in enumerate(run.logs):
        lines = [ln for ln in log.split("\n") if "grad norm" in ln and "[%d] Ed:" % r in ln]
        assert lines and "[%d] Ed: 4," % r in lines[0], lines[:1]           # batch 0 is inside the window: no update, no norm yet
        got.append(float(re.search(r"grad norm (\S+) \(clip", lines[0]).group(1)))
    assert got[0] == got[1] and np.isfinite(got[0]) and got[0] > 0
    args = parse_args(MODEL + ON + SYNTH)
    torch.cuda.set_device(0)
    eng = E.Engine(engine_config_from_args(args), "cuda:0", max_batch=args.batch_size, dtype=args.dtype)
    eng.load_state_dict({k: hashinit.init_tensor(1234, k, tuple(shp)) for k, shp in eng.shapes.items()})
    n, B = 51282, args.batch_size
    d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    news, tabs = d(synth.news_table(1234, n, args.num_words_title)), d(synth.teacher_tables(1234, args.num_teachers, n, args.news_dim))
    batches = []
    for r in range(2):
        imp = synth.impressions(77 + r, 6 * B, n, args.user_log_length, args.npratio + 1)
        batches += [[x[i * B:(i + 1) * B] for x in imp] for i in range(2)]
    for j, (h, m, c, y) in enumerate(batches):
        plan = build_plan(h, c)
        eng.forward_indexed(news, d(h), d(m), d(c), d(y), tabs, plan.to("cuda") if plan is not None else None)
        eng.backward(micro=(j, 4))
    eng.step(args.lr, grad_scale=0.25, max_grad_norm=1.0)
    want = eng.grad_norm()[0]
    eng.scaler.drain(eng)
    assert eng.scaler.skipped == 0 and np.isfinite(want) and want > 0
    rel = abs(got[0] - want) / want
    print("\ngrad norm of the first window: two ranks (run.py's log) %.6g, one engine with the four batches %.6g, rel. difference %.2e"
          % (got[0], want, rel))
    assert rel < 1e-3


# -- (c) file-fed, one rank, the three feed forms -----------------------------------------------------------------------------------
def filefed_runs(base, filefed, form):
    return group("filefed_w1_" + form, lambda: abc(base / ("filefed_w1_" + form), filefed + FORMS[form], 1))


@pytest.mark.parametrize("form", list(FORMS))
def test_filefed_resume(base, filefed, form):
    runs = filefed_runs(base, filefed, form)
    caps = F.expected_caps(F.LINE_COUNTS, 1, F.BATCH, 2)
    assert caps == [17, 17]
    c_equals_a(runs, sum(c // 2 for c in caps), 1)           # windows of 2: the 17th batch (the short one) updates nothing
    for k in ("params", "adam_m", "adam_v", "adam_vmax", "ema", "step_count", "gscale", "skipped"):
        assert np.array_equal(runs["A"].npz[0][k], runs["C"].npz[0][k]), k
    logs_of_a_resume(runs["C"])
    assert runs["C"].logs[0].count("Model saved to") == 1
    if form != "decode_process":          # (the child process's log lines go nowhere)
        # ONE sampler per epoch, seeded with the epoch's number (the first 0 is run.py's count of the samples, before the loader)
        seeds = lambda k: [int(x) for x in re.findall(r"shuffle:True, seed:(\d+)", runs[k].logs[0])]
        assert seeds("A") == [0, 0, 1] and seeds("B") == [0, 0] and seeds("C") == [0, 1]


CKPT = ("model_state_dict", "ema_state_dict", "optimizer_state_dict", "ema", "train_state")


@pytest.mark.parametrize("form", ["producer_thread", "rows_from_host"])
def test_filefed_feed_forms_agree(base, filefed, form):
    """--decode_process: "identical batches"; the resident tables, the de-duplication and the frozen-layer cache: "identical
    results" - through run.py, two epochs, every bit of A's checkpoint against the default form's (no launch of its own).
    rows_from_host: the rows gathered on the host are de-duplicated by the plan the resident feed uses (RowBatch.plan); before
    that this feed encoded every slot, its gradients agreed with the default feed's to summation order only, and Adam turned
    the rounding noise of (nearly) zero gradients into full steps: 47 of 67 tensors differed after 8 updates, max 6.1e-4."""
    first = load(filefed_runs(base, filefed, "decode_process")["A"].dir, "epoch-2.pt")
    other = load(filefed_runs(base, filefed, form)["A"].dir, "epoch-2.pt")
    for key in CKPT:
        _equal(first[key], other[key], "decode_process against %s: %s" % (form, key))


def test_filefed_feeds_agree_without_dedup(base, filefed):
    """--dedup_news False: both feeds encode every slot of a batch, and agree in every bit as well (one launch each)."""
    off = filefed + ["--dedup_news", "False"]
    resident = load(abc(base / "filefed_w1_resident_no_dedup", off, 1, only_a=True)["A"].dir, "epoch-2.pt")
    rows = load(abc(base / "filefed_w1_rows_no_dedup", off + FORMS["rows_from_host"], 1, only_a=True)["A"].dir, "epoch-2.pt")
    for key in CKPT:
        _equal(resident[key], rows[key], "without de-duplication, resident against rows_from_host: " + key)
    # and the de-duplication is not a no-op on these batches: the default form's run ends elsewhere
    first = load(filefed_runs(base, filefed, "decode_process")["A"].dir, "epoch-2.pt")
    w = "student.news_encoder.dense.weight"
    assert not torch.equal(first["model_state_dict"][w], resident["model_state_dict"][w])


# -- (d) file-fed, two ranks ----------------------------------------------------------------------------------------------------------
def test_filefed_two_ranks_resume(base, filefed):
    runs = abc(base / "filefed_w2", filefed, 2)
    for k in "ABC":
        ranks_agree(runs[k], "file-fed, world 2, " + k)
    caps = F.expected_caps(F.LINE_COUNTS, 2, F.BATCH, 2)
    assert caps == [6, 7]
    c_equals_a(runs, sum(c // 2 for c in caps), 2)
    for k in runs["A"].npz[1]:
        assert np.array_equal(runs["A"].npz[1][k], runs["C"].npz[1][k]), "rank 1: C differs from A in " + k
    said = lambda log, r: [int(x) for x in re.findall(r"\[%d\] (\d+) steps this epoch on every rank \(shortest shard\)" % r, log)]
    for r in range(2):
        assert said(runs["A"].logs[r], r) == caps
        assert said(runs["B"].logs[r], r) == caps[:1]
        assert said(runs["C"].logs[r], r) == caps[1:]
    only_rank_0_wrote(runs["A"], ["epoch-1.pt", "epoch-2.pt"], 2)
    only_rank_0_wrote(runs["C"], ["epoch-1.pt", "epoch-2.pt"], 1)
    logs_of_a_resume(runs["C"])
