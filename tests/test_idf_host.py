"""Host checks of the IDF line: the formulas, the penalty weights, the exchange format, the YAML section and the CLIs'
argument handling (snx/idf.py, src/train/config/idf.py, src/train/cli/compute_idf.py).  No GPU."""
import ast
import inspect
import json
import types

import numpy as np
import pytest
import torch

from tests import idf_reference as R


def _ulps(a, b):
    a, b = np.asarray(a, np.float32), np.asarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


# ------------------------------------------------------------------------------------------------ formulas
def test_formulas_at_the_references_cases():
    """ref:scripts/test_idf_math.py:25-55: N = 1000, df in {0, 1, 100, 500, 1000}; IDF falls as df grows and bm25 is
    non-negative.  `smooth` is >= 1 by construction; `standard` goes below zero at df = N (ln(N / (N + 1))), which is why
    sparse query rows drop ids with idf <= 0."""
    from snx.idf import idf_from_counts
    N, dfs = 1000, [0, 1, 100, 500, 1000]
    for sm in ("bm25", "standard", "smooth"):
        got = idf_from_counts(np.asarray(dfs), N, sm)
        assert got.dtype == np.float32
        assert np.array_equal(got.view(np.int32), R.idf(dfs, N, sm).view(np.int32)), sm
        assert all(a > b for a, b in zip(got[:-1], got[1:])), sm
    assert (idf_from_counts(np.asarray(dfs), N, "bm25") >= 0).all()
    assert (idf_from_counts(np.asarray(dfs), N, "smooth") >= 1).all()
    assert idf_from_counts(np.asarray([N]), N, "standard")[0] < 0
    assert float(idf_from_counts(np.asarray([0]), N, "bm25")[0]) == pytest.approx(np.log(1 + 1000.5 / 0.5), rel=1e-7)
    with pytest.raises(ValueError):
        idf_from_counts(np.asarray(dfs), N, "lucene")


# ------------------------------------------------------------------------------------------------ penalty weights
def test_penalty_weights_rules():
    from snx.idf import penalty_weights
    V = 1000
    idf = torch.linspace(0.5, 5.0, V)                          # test_idf_math.py:71
    idf[0], idf[1] = 40.0, -3.0                                # special ids with outlying values: outside min / max
    special, stop = [0, 1, 999], [5, 6, 7, 999]
    w = penalty_weights(idf, special_ids=special, stopword_ids=stop)
    assert w.dtype == torch.float32 and tuple(w.shape) == (V,)
    want = R.penalty_weights(idf.numpy(), special_ids=special, stopword_ids=stop)
    assert np.array_equal(w.numpy().view(np.int32), want.view(np.int32))
    assert (w[special] == 100.0).all()                         # set, also where the id is a stop-word too
    plain = penalty_weights(idf, special_ids=special)
    others = [i for i in range(V) if i not in special and i not in stop]
    assert torch.equal(w[others], plain[others])               # untouched
    for i in (5, 6, 7):                                        # multiplied (test_idf_math.py:123-126)
        assert float(w[i]) == pytest.approx(15.0 * float(plain[i]), rel=2 ** -23)
    # min / max over the real ids: the rarest real token has idf_norm = 1 - O(1e-8), the most common 0
    assert float(plain[2]) == 1.0 and float(plain[998]) == pytest.approx(np.exp(-4.0), rel=1e-6)
    assert float(plain[2]) > float(plain[500]) > float(plain[998])
    with pytest.raises(ValueError):
        penalty_weights(idf, special_ids=[V])
    with pytest.raises(ValueError):
        penalty_weights(torch.ones(3), special_ids=[0, 1, 2])


def _torch_fp32_weights(idf, alpha, stop, stop_penalty):
    lo, hi = idf.min(), idf.max()
    norm = (idf - lo) / (hi - lo + 1e-8)
    w32 = torch.exp(-alpha * norm)
    w32[stop] = w32[stop] * stop_penalty
    return w32, norm


def test_penalty_weights_against_a_torch_fp32_evaluation():
    """float64 then one rounding, against the same expressions in torch fp32, on the reference's own table
    (ref:scripts/test_idf_math.py:71, alpha = 4, stop-words x 15): within 2 fp32 ulp (measured: 2).  The figure is a property
    of this table, not of the expressions: see the next test."""
    from snx.idf import penalty_weights
    idf = torch.linspace(0.5, 5.0, 1000)
    stop = list(range(10, 60))
    got = penalty_weights(idf, alpha=4.0, stopword_ids=stop, stopword_penalty=15.0)
    w32, _ = _torch_fp32_weights(idf, 4.0, stop, 15.0)
    d = _ulps(got.numpy(), w32.numpy())
    print("max ulp distance", int(d.max()))
    assert int(d.max()) <= 2


def test_penalty_weights_against_torch_fp32_on_a_random_table():
    """A random table over [0.2, 9.2] is 5 ulp from the torch-fp32 evaluation (measured), and the error is the fp32
    side's: idf_norm takes three roundings there (difference, denominator, quotient), so the exponent alpha * idf_norm is
    off by up to 3 * 2^-24 * alpha * idf_norm, which exp turns into that RELATIVE error of w -- at most 2 * 3 * alpha *
    idf_norm ulp, an ulp being at least 2^-24 relative -- plus torch's exp (1 ulp), the stop-word product (1/2 ulp) and
    the float64 side's single rounding (1/2 ulp).  The bound is per element and comes from the formats alone."""
    from snx.idf import penalty_weights
    g = torch.Generator().manual_seed(3)
    idf = torch.rand(5000, generator=g) * 9.0 + 0.2
    stop = list(range(10, 60))
    got = penalty_weights(idf, alpha=4.0, stopword_ids=stop, stopword_penalty=15.0)
    w32, norm = _torch_fp32_weights(idf, 4.0, stop, 15.0)
    d = _ulps(got.numpy(), w32.numpy())
    bound = np.ceil(2 * 3 * 4.0 * norm.numpy().astype(np.float64)) + 2
    print("max ulp distance", int(d.max()), "largest bound", int(bound.max()))
    assert (d <= bound).all()


# ------------------------------------------------------------------------------------------------ exchange format
def test_bin_json_round_trip(tmp_path):
    from snx.idf import META_KEYS, idf_to_pt, load_idf, save_idf, save_idf_json
    rng = np.random.default_rng(0)
    w = rng.random(777).astype(np.float32) * 11
    base = tmp_path / "sub" / "idf"
    meta = save_idf(base, w, 12345, "bm25", "hash:777")
    raw = open(str(base) + ".bin", "rb").read()
    assert raw == w.astype("<f4").tobytes()
    on_disk = json.load(open(str(base) + ".json"))
    assert on_disk == meta and set(on_disk) == set(META_KEYS) and len(META_KEYS) == 6
    assert on_disk == {"vocab_size": 777, "num_docs": 12345, "smoothing": "bm25", "tokenizer_name": "hash:777",
                       "dtype": "float32", "byte_order": "little_endian"}
    # what the reference's loader does (ref:tools/idf-compute/load_idf.py:13-24)
    theirs = np.fromfile(str(base) + ".bin", dtype=np.float32, count=on_disk["vocab_size"])
    assert np.array_equal(theirs.view(np.int32), w.view(np.int32))
    back, m2 = load_idf(base)
    assert m2 == meta and back.dtype == np.float32 and np.array_equal(back.view(np.int32), w.view(np.int32))
    # and the reverse: a table written the way the Rust tool writes it (main.rs:213-234)
    other = tmp_path / "rust"
    with open(str(other) + ".bin", "wb") as f:
        for x in w.tolist():
            f.write(np.float32(x).astype("<f4").tobytes())
    with open(str(other) + ".json", "w") as f:
        json.dump({**meta, "smoothing": "standard"}, f, indent=2)
    back2, m3 = load_idf(other)
    assert np.array_equal(back2.view(np.int32), w.view(np.int32)) and m3["smoothing"] == "standard"
    pt = idf_to_pt(w, tmp_path / "idf")
    assert pt.endswith(".pt") and torch.equal(torch.load(pt), torch.from_numpy(w))
    assert np.array_equal(load_idf(pt)[0], w)
    from src.train.data.collator import create_tokenizer
    tok = create_tokenizer("hash:777")
    n = save_idf_json(tmp_path / "idf.json", w, tok)
    table = json.load(open(tmp_path / "idf.json"))
    assert n == len(table) == 777 and table["w10"] == float(w[10]) and table["<pad>"] == float(w[776])
    with open(str(other) + ".bin", "wb") as f:
        f.write(w[:5].tobytes())
    with pytest.raises(ValueError):
        load_idf(other)


# ------------------------------------------------------------------------------------------------ configuration
YAML = """
model: {name: some/dir}
loss: {lambda_q: 0.02}
idf:
  idf_weights_path: out/idf
  idf_alpha: 3.0
  beta: 0.25
  stopword_file: words.txt
  query_mode: idf
"""


def test_idf_config_from_yaml(tmp_path):
    import yaml
    from src.train.config.idf import IdfConfig, load_idf_config
    cfg = load_idf_config(yaml.safe_load(YAML))
    assert cfg == IdfConfig(idf_weights_path="out/idf", idf_smoothing="bm25", idf_alpha=3.0, beta=0.25,
                            special_token_penalty=100.0, stopword_penalty=15.0, stopword_file="words.txt",
                            query_mode="idf", query_idf_path=None)
    assert cfg.doc_only and cfg.enabled
    d = IdfConfig()
    assert (d.idf_weights_path, d.idf_smoothing, d.idf_alpha, d.beta, d.special_token_penalty, d.stopword_penalty,
            d.stopword_file, d.query_mode, d.query_idf_path) == (None, "bm25", 4.0, 0.3, 100.0, 15.0, None, "encoder", None)
    assert load_idf_config({"model": {}}) is None and load_idf_config(None) is None
    over = load_idf_config({"model": {}}, idf_weights="x/idf", query_mode="idf")
    assert over.idf_weights_path == "x/idf" and over.doc_only
    assert load_idf_config(yaml.safe_load(YAML), query_mode="encoder").doc_only is False
    for bad in ({"idf": {"idf_weights_path": "a", "query_mode": "bm25"}}, {"idf": {"idf_weights_path": "a", "alpha": 1}},
                {"idf": {"beta": 0.1}}, {"idf": {"idf_weights_path": "a", "idf_smoothing": "x"}}):
        with pytest.raises(ValueError):
            load_idf_config(bad)
    # the V33 loader ignores the section
    from src.train.cli import train_v33_ddp as cli
    p = tmp_path / "c.yaml"
    p.write_text(YAML)
    args = types.SimpleNamespace(config=str(p), idf_weights=None, query_mode=None,
                                 **{a: None for a, _, _ in cli._OVERRIDES})
    v33 = cli.load_config(args)
    assert v33.loss.lambda_q == 0.02 and not hasattr(v33, "idf")
    assert cli.load_idf_section(args).idf_alpha == 3.0


def test_cli_builds_the_v33_loss_without_the_section(tmp_path):
    from src.model.losses import SPLADELossIDF, SPLADELossV33
    from src.train.cli import train_v33_ddp as cli
    from src.train.config import V33Config
    from src.train.data.collator import create_tokenizer
    p = tmp_path / "c.yaml"
    p.write_text("loss: {lambda_q: 0.02, temperature: 2.0}\n")
    args = types.SimpleNamespace(config=str(p), idf_weights=None, query_mode=None,
                                 **{a: None for a, _, _ in cli._OVERRIDES})
    assert cli.load_idf_section(args) is None
    loss = cli.build_loss(cli.load_config(args), None, create_tokenizer("hash:300"), 300)
    assert type(loss) is SPLADELossV33 and loss.lambda_q == 0.02 and loss.temperature == 2.0
    # main() goes through build_loss with the parsed section, and names no loss class itself
    tree = ast.parse(inspect.getsource(cli.main))
    calls = [ast.unparse(n.func) for n in ast.walk(tree) if isinstance(n, ast.Call)]
    assert "build_loss" in calls and "load_idf_section" in calls
    assert not any(c in ("SPLADELossV33", "SPLADELossIDF") for c in calls)
    # with the section: the IDF loss, the table padded to the model's vocabulary, special ids at the special penalty
    from snx.idf import save_idf
    save_idf(tmp_path / "idf", np.linspace(0.5, 5.0, 290).astype(np.float32), 10, "bm25", "hash:300")
    (tmp_path / "stop.txt").write_text("# comment\nthe\n\nof\n")
    tok = create_tokenizer("hash:300")
    args.idf_weights, args.query_mode = str(tmp_path / "idf"), "idf"
    cfg = cli.load_idf_section(args)
    cfg.stopword_file = str(tmp_path / "stop.txt")
    loss = cli.build_loss(V33Config(), cfg, tok, 300)
    assert type(loss) is SPLADELossIDF and loss.doc_only and loss.beta == 0.3
    w = loss.penalty_weights
    assert tuple(w.shape) == (300,) and float(w[0]) == float(w[1]) == float(w[299]) == 100.0
    the = tok.encode("the", add_special_tokens=False)[0]
    cfg.stopword_file = None
    plain = cli.build_loss(V33Config(), cfg, tok, 300).penalty_weights
    assert float(w[the]) == pytest.approx(15.0 * float(plain[the]), rel=2 ** -23)   # a stop-word: multiplied by 15
    assert sum(float(a) != float(b) for a, b in zip(w, plain)) == 2                 # "the" and "of", nothing else
    assert float(loss.query_idf[295]) == 5.0 and tuple(loss.query_allowed.shape) == (300,)
    assert int(loss.query_allowed[0]) == 0 and int(loss.query_allowed[the]) == 1
    enc = cli.build_loss(V33Config(), cli.load_idf_config({}, str(tmp_path / "idf"), None), tok, 300)
    assert type(enc) is SPLADELossIDF and not enc.doc_only and enc.query_idf is None


def test_cli_flags():
    from src.train.cli import train_v33_ddp as cli
    src = inspect.getsource(cli.parse_args)
    assert '"--idf-weights"' in src and '"--query-mode"' in src


# ------------------------------------------------------------------------------------------------ compute_idf
def test_compute_idf_arguments(tmp_path):
    from src.train.cli import compute_idf as Cc
    f = tmp_path / "a.jsonl"
    f.write_text(json.dumps({"query": "a b", "positive": "c", "negative": "", "text": None, "other": "zz"}) + "\n"
                 + "not json\n\n" + json.dumps({"document": "d e f", "text": "g"}) + "\n" + json.dumps([1, 2]) + "\n")
    a = Cc.parse_args(["--input", str(tmp_path / "*.jsonl"), "--tokenizer", "hash:100"])
    assert a.files == [str(f)] and a.smoothing == "bm25" and a.output == "outputs/idf_weights/idf" and a.batch_docs == 4096
    assert list(Cc.documents(a.files)) == ["a b", "c", "g", "d e f"]       # empty and missing fields are no documents
    for bad in (["--input", str(tmp_path / "*.jsonl")],                                           # no tokenizer
                ["--input", str(tmp_path / "none*.jsonl"), "--tokenizer", "hash:100"],            # no files
                ["--input", str(f), "--tokenizer", "hash:100", "--smoothing", "lucene"],
                ["--input", str(f), "--tokenizer", "hash:100", "--batch-docs", "0"]):
        with pytest.raises(SystemExit):
            Cc.parse_args(bad)
    from src.train.data.collator import create_tokenizer
    assert Cc.tokenizer_vocab_size(create_tokenizer("hash:100")) == 100


def test_eval_benchmark_doc_only_arguments():
    from src.train.cli import eval_benchmark as E
    a = E.parse_args(["--benchmark-dir", "x", "--methods", "sparse,doc_only", "--idf", "out/idf"])
    assert a.methods == ["sparse", "doc_only"] and a.idf == "out/idf"
    assert "doc_only" not in E.METHODS and E.parse_args(["--benchmark-dir", "x"]).idf is None
    with pytest.raises(SystemExit):
        E.parse_args(["--benchmark-dir", "x", "--methods", "doc_only"])


def test_encode_for_query_with_idf():
    """The inference-free query dictionary: the model is not run (there is none here)."""
    from benchmark.encoders import NeuralSparseEncoderV33, special_token_ids
    from src.train.data.collator import create_tokenizer
    tok = create_tokenizer("hash:300")
    enc = NeuralSparseEncoderV33.__new__(NeuralSparseEncoderV33)
    enc.tokenizer, enc.query_max_length, enc.device = tok, 16, "cpu"
    enc.special_token_ids = special_token_ids(tok)
    enc._token_lookup = list(tok.convert_ids_to_tokens(list(range(300))))
    idf = np.linspace(0.0, 3.0, 300).astype(np.float32)
    out = enc.encode_for_query("alpha beta alpha", idf=idf)
    ids = tok.encode("alpha beta", add_special_tokens=False)
    assert out == {f"w{i}": float(idf[i]) for i in ids}
    assert enc.encode_for_query("alpha beta", idf={f"w{ids[0]}": 2.5}) == {f"w{ids[0]}": 2.5}
