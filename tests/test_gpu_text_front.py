"""The shared tail of the GPU tokenizers' ``encode_rows`` (``RowTokenizer._finish_rows``, snx/_tokenizer.py) at the smallest
batches where the host-row scatter can go wrong, for both models: ptr and ids against the ``device="cpu"`` restatement,
bit for bit."""
import pytest
import torch

from tests import unigram_reference, wordpiece_reference

pytestmark = pytest.mark.gpu


def _load(model, device):
    if model == "wordpiece":
        from snx.wordpiece import WordPieceTokenizer
        return WordPieceTokenizer.from_pretrained(wordpiece_reference.fixture_dir(), device=device)
    from snx.unigram import UnigramTokenizer
    return UnigramTokenizer.from_pretrained(unigram_reference.fixture_dir(), device=device)


@pytest.fixture(scope="module", params=["wordpiece", "unigram"], ids=["wordpiece-g23", "unigram-g24"])
def pair(request):
    return _load(request.param, "cuda"), _load(request.param, "cpu")


def assert_same(gpu, cpu, texts, max_length, host_rows):
    ptr, ids = gpu.encode_rows(texts, max_length)
    stats = dict(gpu.last_stats)
    want_ptr, want_ids = cpu.encode_rows(texts, max_length)
    assert ptr.is_cuda and ids.is_cuda and ptr.dtype == ids.dtype == torch.long
    assert ptr.cpu().tolist() == want_ptr.tolist()
    assert ids.cpu().tolist() == want_ids.tolist()
    assert (stats["rows"], stats["host_rows"]) == (len(texts), host_rows)


def added(tok):
    """Two added tokens' texts; a row that holds one is the host's."""
    a = sorted(tok._added)
    assert len(a) >= 2
    return a[0], a[-1]


@pytest.mark.parametrize("max_length", (None, 8), ids=("none", "8"))
def test_host_rows_on_both_edges_of_a_batch_with_an_empty_and_a_workspace_row(pair, max_length):
    gpu, cpu = pair
    first, last = added(gpu)
    long_row = "hello world, again and again. " * 140           # 4,200 code points: past the LDS forms of both models
    assert len(long_row) >= 4097
    texts = [f"hello {first} world", "", "an ordinary short row", long_row, f"{last} at the front"]
    assert_same(gpu, cpu, texts, max_length, 2)


def test_every_row_is_a_host_row(pair):
    gpu, cpu = pair
    first, last = added(gpu)
    texts = [first, f"a {last} b {first}", f"{last}{last}", f"tail {first}"]
    assert_same(gpu, cpu, texts, None, len(texts))
    assert_same(gpu, cpu, texts, 3, len(texts))


def test_only_empty_rows(pair):
    gpu, cpu = pair
    assert_same(gpu, cpu, ["", "", ""], None, 0)
    assert_same(gpu, cpu, [""], 2, 0)
    assert gpu.encode_rows(["", ""])[1].tolist() == [gpu._bos, gpu._eos] * 2


def test_no_rows(pair):
    gpu, cpu = pair
    ptr, ids = gpu.encode_rows([])
    assert ptr.is_cuda and ptr.tolist() == [0] and ids.is_cuda and ids.numel() == 0 and ids.dtype == torch.long
    assert gpu.last_stats["rows"] == gpu.last_stats["host_rows"] == 0
    want_ptr, want_ids = cpu.encode_rows([])
    assert want_ptr.tolist() == [0] and want_ids.numel() == 0
