"""post_train_kd.py fed from files (tests/kd_files.py): the script against the API, the oracle, its own files and two ranks.

Every engine is 2 layers x 256 wide (the stage-0 teacher of the pipeline test: 3), a run is at most 6 steps of 4 samples.
  (a) the checkpoint the script writes is torch.equal, key by key, to a hand loop over Stage1Engine written out here - tokens by
      tests/wordpiece_ref.py, indices by kd_files.expected_indices, step keywords spelled out - in every optimiser form;
  (b) that hand loop's first step (dropout off) against oracle.newsrec_oracle.distill_fwd / distill_bwd;
  (c) --mode export against Stage1Engine.encode_table and against the oracle's news encoder;
  (d) stage 0 -> export -> stage 1 -> run.py --use_pretrain_model through the files each of them writes;
  (e) the script at two ranks (tests/workers/kd_rank.py, gloo, both on cuda:0) against a one-process loop of two engines whose
      gradients are added in fp32.
The script runs in process (post_train_kd.train(parse_args([...])), --enable_hvd False) except in (e)."""
import logging
import os
import pickle
import re
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import hashinit                                   # noqa: E402
import kd_files as F                              # noqa: E402
import post_train_kd as K                         # noqa: E402
from model_bert import reference_init             # noqa: E402
from oracle import newsrec_oracle as O            # noqa: E402
from stage1 import Stage1Engine                   # noqa: E402
from test_n2_gpu import VEC_TOL                   # noqa: E402
from test_stage1_gpu import GTOL, TOL             # noqa: E402

DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "tiny-newsrec_amd")
WORKER = os.path.join(ROOT, "tests", "workers", "kd_rank.py")
LIMIT = 300.0                                     # s per rank process: a guard against hangs, not a measurement
LR, LR_BERT = 1e-3, 1e-4                          # (the notebook's 1e-5 / 1e-6 would hardly move a weight in six steps)
RATES = ["--lr", str(LR), "--pretrain_lr", str(LR_BERT)]
STUDENT = ["--num_hidden_layers", "2", "--bert_trainable_layer", "0", "1"]
ALL_ON = ["--max_grad_norm", "1.0", "--weight_decay", "0.01", "--warmup_steps", "2", "--lr_decay_steps", "5", "--ema_decay", "0.9",
          "--ema_warmup", "True"]
ALL_ON_KW = dict(max_grad_norm=1.0, weight_decay=0.01, warmup_steps=2, lr_decay_steps=5, ema_decay=0.9, ema_warmup=True)
# name -> (stage, the script's flags, Engine.step's keywords they stand for)
CASES = {"stage1_plain": (1, [], {}),
         "stage0": (0, ["--save_steps", "2"], {}),
         "stage1_all_on": (1, ALL_ON, ALL_ON_KW),
         "stage1_lamb": (1, ["--optimizer", "lamb"], dict(lamb=True))}


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The corpus, vocabulary and config of kd_files, two hash-made teacher pickles, and the reference tables."""
    d = tmp_path_factory.mktemp("kd_files")
    z = type("Files", (), {})()
    z.dir, z.flags = str(d), F.write_inputs(d)
    for i in range(2):
        for which in ("title", "body"):
            with open(os.path.join(z.dir, "teacher_%s_emb_%d.pkl" % (which, i)), "wb") as f:
                pickle.dump(hashinit.hash_normal(70 + i, which, (F.N_DOCS, F.NEWS_DIM)), f)
    z.title, z.body = F.tables(d)
    z.runs = {}
    return z


def teacher_tables(dirname, n):
    out = []
    for which in ("title", "body"):
        arrs = []
        for i in range(n):
            with open(os.path.join(dirname, "teacher_%s_emb_%d.pkl" % (which, i)), "rb") as f:
                arrs.append(np.asarray(pickle.load(f), dtype=np.float32))
        out.append(np.stack(arrs, 0) if n else np.zeros((1, 1, F.NEWS_DIM), np.float32))
    return out


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def make_engine(files, stage, dtype, seed=F.SEED, rank=0, dropout=(0.1, 0.1), n_layers=2, trainable=(0, 1)):
    """What the script builds on its file-fed branch: construction, reference_init, the body's rel-pos table, dropout."""
    eng = Stage1Engine(n_layers=n_layers, trainable_layers=list(trainable), num_teachers=2 if stage == 1 else 0, device=DEV, dtype=dtype,
                       **F.engine_dims(files.dir))
    reference_init(eng.title, seed)
    eng.body.refresh_rel()
    eng.set_dropout(dropout[0], dropout[1], seed * 1000003 + rank)
    return eng


def ckpt_of(eng, stage, ema=None):
    """What the script's checkpoint must hold, from the engine's own state_dict()."""
    strip = (lambda sd: {k: v.cpu() for k, v in sd.items()}) if stage == 1 else \
        (lambda sd: {k[len("student."):]: v.cpu() for k, v in sd.items()})
    out = {"model_state_dict": strip(eng.state_dict())}
    if ema is not None:
        out["ema_state_dict"] = strip(eng.ema_state_dict())
        out["ema"] = dict(ema, updates=eng.ema_updates)
    return out


def hand_loop(files, stage, dtype, step_kw, snapshots=(), teacher_dir=None):
    """Six steps of the epoch as the script documents them -> (engine, {step: checkpoint dict} for `snapshots`)."""
    eng = make_engine(files, stage, dtype)
    tt, tb = teacher_tables(teacher_dir or files.dir, 2 if stage == 1 else 0)
    d_title, d_body, d_tt, d_tb = dev(files.title), dev(files.body), dev(tt), dev(tb)
    label = torch.zeros(F.BATCH, dtype=torch.int64, device=DEV)
    snaps = {}
    batches = F.expected_indices(F.SEED, 0, 1, 0, F.N_DOCS, F.BATCH, F.K)
    assert len(batches) == 6
    for cnt, idx in enumerate(batches, 1):
        eng.forward_indexed(d_title, d_body, dev(idx), label, d_tt, d_tb)
        eng.backward()
        eng.step(LR, lr_bert=LR_BERT, amsgrad=False, **step_kw)
        if cnt in snapshots:
            snaps[cnt] = ckpt_of(eng, stage)
    if eng.title.scaler.enabled:
        eng.title.scaler.drain(eng.title)
    return eng, snaps


def equal_ckpt(got, want, what):
    assert list(got) == list(want), (what, list(got), list(want))
    for part in want:
        if part == "ema":
            assert got[part] == want[part], (what, got[part], want[part])
            continue
        assert list(got[part]) == list(want[part]), (what, part)
        bad = [k for k in want[part] if not torch.equal(got[part][k], want[part][k])]
        assert not bad, "%s: %s differs in %d of %d tensors, first %s (max |diff| %.3e)" % (
            what, part, len(bad), len(want[part]), bad[0], float((got[part][bad[0]] - want[part][bad[0]]).abs().max()))


def script_run(files, case, dtype, caplog):
    """post_train_kd.train() for a case of CASES, once per module -> (save dir, log text, ran_joint)."""
    key = (case, dtype)
    if key not in files.runs:
        stage, flags, _ = CASES[case]
        save = os.path.join(files.dir, "out_%s_%s" % (case, dtype))
        argv = files.flags + RATES + STUDENT + flags + ["--stage", str(stage), "--num_teachers", "2", "--teacher_emb_dir", files.dir,
                                                       "--save_dir", save, "--dtype", dtype, "--enable_hvd", "False"]
        caplog.clear()
        with caplog.at_level(logging.INFO):
            eng = K.train(K.parse_args(argv))
        torch.cuda.synchronize()
        files.runs[key] = (save, "\n".join(r.getMessage() for r in caplog.records), bool(eng.ran_joint))
        del eng
    return files.runs[key]


# -- (a) the script equals the API ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,dtype", [(c, "fp16") for c in CASES] + [("stage1_plain", "bf16")])
def test_script_checkpoint_equals_the_hand_loop(files, case, dtype, caplog):
    stage, flags, step_kw = CASES[case]
    save, log, ran_joint = script_run(files, case, dtype, caplog)
    name = "first_stage_2_layer.pt" if stage == 1 else "DP_2_layer.pt"
    got = torch.load(os.path.join(save, name), map_location="cpu")
    eng, snaps = hand_loop(files, stage, dtype, step_kw, snapshots=(2, 4, 6) if stage == 0 else ())
    torch.cuda.synchronize()
    ema = dict(decay=0.9, warmup=True) if "ema_decay" in step_kw else None
    want = ckpt_of(eng, stage, ema)
    sd = got["model_state_dict"]
    if stage == 1:
        assert all(k.startswith("student.news_encoder.") or k.startswith("transform_matrix.") for k in sd) and \
            {"transform_matrix.0.weight", "transform_matrix.1.bias", "student.news_encoder.dense.weight"} <= set(sd)
    else:
        assert all(k.startswith("news_encoder.") for k in sd) and "news_encoder.dense.weight" in sd
    assert (ema is not None) == ("ema_state_dict" in got)
    equal_ckpt(got, want, "%s %s" % (case, dtype))
    if stage == 0:           # the periodic checkpoints (cell 16), written before the scaler is drained
        assert sorted(os.listdir(save)) == ["DP_2_layer.pt", "DP_2_layer_2.pt", "DP_2_layer_4.pt", "DP_2_layer_6.pt"]
        for cnt, snap in snaps.items():
            equal_ckpt(torch.load(os.path.join(save, "DP_2_layer_%d.pt" % cnt), map_location="cpu"), snap, "stage 0, step %d" % cnt)
    else:
        assert os.listdir(save) == [name]
    # the log: six steps of four, the form of the step as the engine took it, the dropout of the config
    assert [int(x) for x in re.findall(r"\[0\] ed: (\d+),", log)] == [4, 8, 12, 16, 20, 24], log[-2000:]
    assert ("[0] stage %d: %s" % (stage, "joint passes" if eng.ran_joint else "per-pass")) in log and ran_joint == eng.ran_joint
    assert "train-mode dropout: hidden 0.1, attention probabilities 0.1" in log and "nan" not in log.lower()
    assert "not found, random init" in log
    # and the run did train: the weights left where reference_init put them
    fresh = ckpt_of(make_engine(files, stage, dtype), stage)["model_state_dict"]
    moved = [k for k in fresh if not torch.equal(fresh[k], sd[k])]
    assert any("encoder.layer.0." in k for k in moved) and any(k.endswith("news_encoder.dense.weight") for k in moved)
    if "lamb" in step_kw:
        assert "trust ratio min" in log
    if "max_grad_norm" in step_kw:
        assert "grad norm" in log and "lr x" in log


def test_fewer_documents_than_a_batch_is_said(files, tmp_path, caplog):
    """Three documents, batch 4: (3 // 1) // 4 = 0 steps.  The checkpoint holds reference_init's weights - and the log says so."""
    with open(os.path.join(files.dir, "docs_filter.tsv"), encoding="utf-8") as f:
        lines = f.readlines()[:3]
    (tmp_path / "three.tsv").write_text("".join(lines), encoding="utf-8")
    flags = list(files.flags)
    flags[flags.index("--corpus_path") + 1] = str(tmp_path / "three.tsv")
    with caplog.at_level(logging.INFO):
        K.train(K.parse_args(flags + STUDENT + ["--stage", "0", "--save_dir", str(tmp_path / "out"), "--enable_hvd", "False"]))
    warned = [r.getMessage() for r in caplog.records if r.levelno == logging.WARNING and "no step is taken" in r.getMessage()]
    assert len(warned) == 1 and "3 documents" in warned[0] and "batch of 4" in warned[0], warned
    assert not any("ed:" in r.getMessage() for r in caplog.records)
    got = torch.load(str(tmp_path / "out" / "DP_2_layer.pt"), map_location="cpu")
    equal_ckpt(got, ckpt_of(make_engine(files, 0, "fp16"), 0), "no step")


# -- (b) the first step against the oracle -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["fp16", "bf16"])
def test_first_step_against_the_oracle(files, dtype):
    eng = make_engine(files, 1, dtype, dropout=(0.0, 0.0))
    tt, tb = teacher_tables(files.dir, 2)
    idx = F.expected_indices(F.SEED, 0, 1, 0, F.N_DOCS, F.BATCH, F.K, 1)[0]
    assert F.EMPTY_BODY in idx[:, 0] and F.EMPTY_TITLE in idx
    label = np.zeros(F.BATCH, np.int64)
    losses, score = eng.forward_indexed(dev(files.title), dev(files.body), dev(idx), dev(label), dev(tt), dev(tb))
    eng.backward()
    torch.cuda.synchronize()
    P = {k: v.cpu().numpy() for k, v in eng.state_dict().items()}
    cfg = dict(n_layers=2, heads=F.HEADS, trainable_layers=[0, 1])
    out = O.distill_fwd(P, cfg, files.title.astype(np.int64)[idx], files.body.astype(np.int64)[idx[:, 0]], label,
                        [tt[i][idx] for i in range(2)], [tb[i][idx[:, 0]] for i in range(2)])
    G = O.distill_bwd(P, cfg, out)
    l = losses.cpu().numpy()
    got = dict(distill_loss=l[0], target_loss=l[1], emb_loss=l[2], total_loss=float(eng.total_loss().item()))
    tol = TOL[dtype]
    for k, v in got.items():
        print("\n[kd files, step 1, %s] %s: got %.6f ref %.6f" % (dtype, k, v, float(out[k])), end="")
        assert abs(v - float(out[k])) <= tol * max(1.0, abs(float(out[k]))), k
    sc, ref = score.cpu().numpy(), out["student_score"]
    print("\n   score max|err| %.3e (|ref| max %.2f)" % (np.abs(sc - ref).max(), np.abs(ref).max()))
    assert np.abs(sc - ref).max() <= tol * max(1.0, np.abs(ref).max())
    assert set(eng.title.grads) == set(G), set(eng.title.grads) ^ set(G)
    worst = 0.0
    for k in eng.title.grads:
        g, r = eng.grad(k).cpu().numpy(), G[k]
        if k.endswith("self.key.bias") or k.endswith("att_fc2.bias"):
            assert np.abs(g).max() < 1e-3          # mathematical no-ops: rounding noise only (tests/test_stage1_gpu.py)
            continue
        rn = np.sqrt((r.astype(np.float64) ** 2).sum())
        err = np.sqrt(((g - r).astype(np.float64) ** 2).sum()) / (rn + 1e-12)
        worst = max(worst, err)
        assert err < GTOL[dtype], "%s: relative L2 error %.3e (norm %.3e)" % (k, err, rn)
    print("   worst gradient relative L2 error %.3e" % worst)


# -- (c) export against encode_table and the oracle ----------------------------------------------------------------------------------
def test_export_against_encode_table_and_the_oracle(files, caplog):
    dtype = "fp16"
    save, _, _ = script_run(files, "stage0", dtype, caplog)
    ckpts = [os.path.join(save, "DP_2_layer_2.pt"), os.path.join(save, "DP_2_layer.pt")]
    out = os.path.join(files.dir, "export")
    argv = files.flags + STUDENT + ["--stage", "0", "--mode", "export", "--ckpt_paths"] + ckpts + \
        ["--save_dir", out, "--dtype", dtype, "--enable_hvd", "False"]
    K.train(K.parse_args(argv))
    assert sorted(os.listdir(out)) == sorted("teacher_%s_emb_%d.pkl" % (w, i) for w in ("title", "body") for i in range(2))
    # a fresh engine that HAS had dropout switched on: encode_table runs with train=False and must not draw a mask
    eng = make_engine(files, 0, dtype, seed=3, dropout=(0.1, 0.1))
    assert eng.body.N_alloc == 4 and F.N_DOCS == 6 * 4 + 3                 # seven passes over the bodies, the last one of three
    tabs = {"title": files.title, "body": files.body}
    embs = {}
    for i, ck in enumerate(ckpts):
        sd = torch.load(ck, map_location="cpu")["model_state_dict"]
        eng.load_state_dict({"student." + k: v for k, v in sd.items()})
        P = {"student." + k: v.numpy() for k, v in sd.items()}
        for which in ("title", "body"):
            with open(os.path.join(out, "teacher_%s_emb_%d.pkl" % (which, i)), "rb") as f:
                emb = pickle.load(f)
            assert isinstance(emb, np.ndarray) and emb.dtype == np.float32 and emb.shape == (F.N_DOCS, F.NEWS_DIM)
            again = eng.encode_table(dev(tabs[which]), which).cpu().numpy()
            assert np.array_equal(emb, again), (i, which, float(np.abs(emb - again).max()))
            want, _ = O.news_encoder_fwd(P, tabs[which].astype(np.int64), 2, F.HEADS)
            err = float((np.abs(emb - want) / np.maximum(1.0, np.abs(want))).max())
            print("\n[kd files export %s %d] max |err| / max(1, |ref|) %.2e (|ref| max %.2f)" % (which, i, err, np.abs(want).max()), end="")
            assert err <= VEC_TOL[dtype], (i, which, err)
            embs[which, i] = emb
    assert not np.array_equal(embs["title", 0], embs["title", 1])             # two checkpoints, two teachers
    assert eng.title.drop_calls == 0 and eng.body.drop_calls == 0


# -- (d) the pipeline through its files ----------------------------------------------------------------------------------------------
def test_pipeline_through_its_files(files, tmp_path, monkeypatch):
    import json

    import filefed_data
    import model_bert
    import parameters
    import run
    common = files.flags + RATES + ["--dtype", "fp16", "--enable_hvd", "False"]
    s0 = str(tmp_path / "stage0")
    K.train(K.parse_args(common + ["--stage", "0", "--num_hidden_layers", "3", "--bert_trainable_layer", "1", "2", "--save_steps", "3",
                                   "--save_dir", s0]))
    ckpts = [os.path.join(s0, "DP_3_layer_3.pt"), os.path.join(s0, "DP_3_layer.pt")]
    emb_dir = str(tmp_path / "teachers")
    K.train(K.parse_args(common + ["--stage", "0", "--num_hidden_layers", "3", "--bert_trainable_layer", "1", "2", "--mode", "export",
                                   "--ckpt_paths"] + ckpts + ["--save_dir", emb_dir]))
    exported = teacher_tables(emb_dir, 2)
    assert exported[0].shape == exported[1].shape == (2, F.N_DOCS, F.NEWS_DIM) and np.isfinite(exported[0]).all()
    # stage 1 reads them: a spy on the loader (it returns what the product's function returned)
    seen, real = [], K.load_teacher_tables

    def spy(*a, **kw):
        seen.append(real(*a, **kw))
        return seen[-1]
    monkeypatch.setattr(K, "load_teacher_tables", spy)
    s1 = str(tmp_path / "stage1")
    K.train(K.parse_args(common + STUDENT + ["--stage", "1", "--num_teachers", "2", "--teacher_emb_dir", emb_dir, "--save_dir", s1]))
    assert len(seen) == 1 and np.array_equal(seen[0][0], exported[0]) and np.array_equal(seen[0][1], exported[1])
    first = torch.load(os.path.join(s1, "first_stage_2_layer.pt"), map_location="cpu")["model_state_dict"]
    want, _ = hand_loop(files, 1, "fp16", {}, teacher_dir=emb_dir)
    equal_ckpt({"model_state_dict": first}, ckpt_of(want, 1), "stage 1 on the exported teachers")
    # run.py starts from it.  Its encoder is built from the config alone, so the config run.py reads names the 72 positions the
    # first stage trained with (post_train_kd.py lengthens the table to --max_body_len by itself)
    d = str(tmp_path / "run")
    os.makedirs(d)
    embs, tckpts, _ = filefed_data.run_py_inputs(d)
    with open(os.path.join(files.dir, "config.json")) as f:
        cfg = dict(json.load(f), max_position_embeddings=F.LB)
    with open(os.path.join(d, "config_run.json"), "w") as f:
        json.dump(cfg, f)
    made, construct = [], model_bert.Model.__init__

    def keeping(self, *a, **kw):
        construct(self, *a, **kw)
        made.append(self)
    monkeypatch.setattr(model_bert.Model, "__init__", keeping)
    argv = ["--mode", "train", "--batch_size", "4", "--num_words_title", "30", "--news_dim", "256", "--num_student_layers", "2",
            "--bert_trainable_layer", "0", "1", "--num_teachers", "2", "--user_log_mask", "False", "--coef", "0.2", "--model", "NAML",
            "--model_type", "tnlrv3", "--enable_hvd", "False", "--epochs", "1", "--lr", "0", "--pretrain_lr", "0",
            "--train_data_dir", os.path.join(filefed_data.GOLDEN, "data"), "--filename_pat", "behaviors_np4_*.tsv",
            "--tokenizer_name", os.path.join(files.dir, "vocab.txt"), "--config_name", os.path.join(d, "config_run.json"),
            "--model_name", os.path.join(d, "none.bin"), "--allow_random_init", "True", "--use_pretrain_model", "True",
            "--pretrain_model_path", os.path.join(s1, "first_stage_2_layer.pt"), "--model_dir", os.path.join(d, "out"),
            "--teacher_emb_paths"] + embs + ["--teacher_ckpts"] + tckpts
    run.train(parameters.parse_args(argv))
    torch.cuda.synchronize()
    model = made[-1]
    mine = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    student = {k: v for k, v in first.items() if k.startswith("student.")}
    # every student.* key of the first stage has a place in run.py's model; what the model has beyond them is the user encoder
    assert set(student) <= set(mine), sorted(set(student) - set(mine))[:5]
    assert {k for k in mine if k.startswith("student.") and k not in student} == {k for k in mine if k.startswith("student.user_encoder.")}
    assert set(first) - set(student) == {k for k in first if k.startswith("transform_matrix.")}
    # both rates 0: the steps of the epoch ran (the checkpoint is there) and the weights are still the first stage's, bit for bit
    bad = [k for k in student if not torch.equal(mine[k], student[k])]
    assert not bad, bad[:5]
    saved = torch.load(os.path.join(d, "out", "epoch-1.pt"), map_location="cpu")["model_state_dict"]
    assert all(torch.equal(saved[k], student[k]) for k in student)


# -- (e) two ranks -------------------------------------------------------------------------------------------------------------------
def launch(out_dir, flags, world, port):
    """kd_rank.py once per rank; both are polled, and when one exits non-zero the other is killed at once."""
    os.makedirs(out_dir, exist_ok=True)
    procs, logs, t0 = [], [], time.time()
    for r in range(world):
        env = dict(os.environ, RANK=str(r), WORLD_SIZE=str(world), LOCAL_RANK="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        logs.append(open(os.path.join(out_dir, "rank%d.log" % r), "w"))
        procs.append(subprocess.Popen([sys.executable, "-u", WORKER, out_dir] + flags, env=env, cwd=PKG, stdout=logs[-1],
                                      stderr=subprocess.STDOUT))
    tail = lambda r: open(os.path.join(out_dir, "rank%d.log" % r)).read()[-4000:]
    bad = None
    try:
        while bad is None and any(p.poll() is None for p in procs):
            for r, p in enumerate(procs):
                if p.poll() not in (None, 0):
                    bad = "rank %d exited with status %s\n%s" % (r, p.returncode, tail(r))
                    break
            else:
                if time.time() - t0 > LIMIT:
                    bad = "no end after %.0f s\n%s" % (LIMIT, "\n".join(tail(r) for r in range(world)))
                else:
                    time.sleep(0.02)
        for r, p in enumerate(procs):
            if bad is None and p.returncode != 0:
                bad = "rank %d exited with status %s\n%s" % (r, p.returncode, tail(r))
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
            p.wait()
        for f in logs:
            f.close()
    if bad is not None:
        pytest.fail(bad, pytrace=False)
    return [dict(np.load(os.path.join(out_dir, "rank%d.npz" % r))) for r in range(world)], [tail(r) for r in range(world)]


def test_two_ranks_equal_two_engines_in_one_process(files, tmp_path):
    import engine as E
    on = ["--max_grad_norm", "1.0", "--weight_decay", "0.01"]
    flags = files.flags + RATES + STUDENT + on + ["--stage", "1", "--num_teachers", "2", "--teacher_emb_dir", files.dir, "--save_dir",
                                                  str(tmp_path / "save"), "--dtype", "fp16", "--enable_hvd", "True"]
    npz, logs = launch(str(tmp_path / "out"), flags, 2, 29981)
    a, b = npz
    for k in a:
        assert a[k].dtype == b[k].dtype and np.array_equal(a[k], b[k]), "rank 0 and rank 1 differ in " + k
    steps = F.steps_per_epoch(F.N_DOCS, 2, F.BATCH)
    assert steps == 3 and int(a["step_count"]) + int(a["skipped"]) == 3
    for r, log in enumerate(logs):
        assert [int(x) for x in re.findall(r"\[%d\] ed: (\d+)," % r, log)] == [4, 8, 12], log[-2000:]
        assert ("Model saved to" in log) == (r == 0)
    assert os.listdir(str(tmp_path / "save")) == ["first_stage_2_layer.pt"]
    # one process, two engines, the ranks' indices and dropout seeds; the two gradients added in fp32 (a + b = b + a: gloo's bits)
    units = E.Engine.WGRAD_UNITS
    E.Engine.WGRAD_UNITS = 2                       # as the script sets it for more than one rank, before the engines are built
    try:
        engs = [make_engine(files, 1, "fp16", rank=r) for r in range(2)]
        tt, tb = teacher_tables(files.dir, 2)
        d_title, d_body, d_tt, d_tb = dev(files.title), dev(files.body), dev(tt), dev(tb)
        label = torch.zeros(F.BATCH, dtype=torch.int64, device=DEV)
        batches = [F.expected_indices(F.SEED, r, 2, 0, F.N_DOCS, F.BATCH, F.K) for r in range(2)]
        for s in range(steps):
            for r, eng in enumerate(engs):
                eng.forward_indexed(d_title, d_body, dev(batches[r][s]), label, d_tt, d_tb)
                eng.backward(after_bucket=lambda i: None)          # the bucket-by-bucket form of the backward, as under GradSync
            total = engs[0].title.flat_g + engs[1].title.flat_g
            for eng in engs:
                eng.title.flat_g.copy_(total)
                eng.step(LR, grad_scale=0.5, lr_bert=LR_BERT, amsgrad=False, max_grad_norm=1.0, weight_decay=0.01, warmup_steps=0,
                         lr_decay_steps=0)
        for eng in engs:
            eng.title.scaler.drain(eng.title)
        torch.cuda.synchronize()
    finally:
        E.Engine.WGRAD_UNITS = units
    for r, eng in enumerate(engs):
        t = eng.title
        want = dict(params=t.flat[True], adam_m=t.adam_m, adam_v=t.adam_v, adam_vmax=t.adam_vmax)
        for k, v in want.items():
            got = torch.from_numpy(a[k])
            assert torch.equal(got, v.cpu()), "%s: the script at two ranks differs from engine %d of the hand loop in %d elements, max %.3e" % (
                k, r, int((got != v.cpu()).sum()), float((got - v.cpu()).abs().max()))
        assert int(a["step_count"]) == t.step_count and float(a["gscale"]) == float(t.gscale) and int(a["skipped"]) == t.scaler.skipped
    fresh = make_engine(files, 1, "fp16").title.flat[True].cpu()
    assert not torch.equal(fresh, torch.from_numpy(a["params"]))                         # and it trained
