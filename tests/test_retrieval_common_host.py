"""Host checks of the plumbing the sections of snx.retrieval share (snx/retrieval/_common.py): the query-slice iterator,
the three step rules that feed it, the CSR-rows normaliser behind exclusion_csr / relevance_csr and the targets
validator.  No GPU: the sizing calls of the C interface are host functions, and the validators take CPU tensors."""
import pytest

torch = pytest.importorskip("torch")


def test_slices_cover_the_queries_in_order():
    from snx.retrieval._common import slices
    assert list(slices(0, 2)) == []
    assert list(slices(1, 2)) == [(0, 1)]
    assert list(slices(5, 2)) == [(0, 2), (2, 2), (4, 1)]
    assert list(slices(5, 8)) == [(0, 5)]                          # a step larger than nq: one launch
    assert list(slices(4, 2)) == [(0, 2), (2, 2)]


def test_step_rules_equal_their_arithmetic_over_the_sizing_calls():
    from snx import fn
    from snx.retrieval._common import step_blocks, step_bytes_mean, step_bytes_per_query
    # bytes budget over the ONE-query sizing value (SparseIndex.search / search_band)
    name = "snx_sparse_search_workspace_bytes"
    one = int(fn(name)(1, 300, 7, 128))
    assert one > 0
    assert step_bytes_per_query(name, 2 * one, 5, 300, 7, 128) == 2
    assert step_bytes_per_query(name, 3 * one - 1, 5, 300, 7, 128) == 2
    assert step_bytes_per_query(name, 3 * one, 5, 300, 7, 128) == 3
    assert step_bytes_per_query(name, one - 1, 5, 300, 7, 128) == 1          # never less than one query
    assert step_bytes_per_query(name, 1 << 40, 5, 300, 7, 128) == 5          # never more than nq
    assert step_bytes_per_query(name, 1 << 40, 0, 300, 7, 128) == 1          # a step is a range() step: >= 1
    band = "snx_sparse_search_band_workspace_bytes"
    assert step_bytes_per_query(band, 2 * int(fn(band)(1, 300, 9, 128)), 5, 300, 9, 128) == 2
    # bytes budget over the nq-query sizing value, divided rounding up (DenseIndex)
    name = "snx_dense_search_workspace_bytes"
    total = int(fn(name)(5, 300, 7, 128))
    per_q = -(-total // 5)
    assert total > 0 and per_q * 5 >= total > (per_q - 1) * 5
    assert step_bytes_mean(name, 2 * per_q, 5, 300, 7, 128) == 2
    assert step_bytes_mean(name, 2 * per_q - 1, 5, 300, 7, 128) == 1
    assert step_bytes_mean(name, per_q // 2, 5, 300, 7, 128) == 1
    assert step_bytes_mean(name, 1 << 40, 5, 300, 7, 128) == 5
    assert step_bytes_mean(name, 1 << 40, 0, 300, 7, 128) == 1              # sized as one query
    # workgroup budget over the chunks of the corpus (SparseIndex.first_relevant)
    assert step_blocks(6, 300, 128) == 2                                    # 3 chunks, the last partial
    assert step_blocks(6, 256, 128) == 3
    assert step_blocks(6, 300, 16384) == 6
    assert step_blocks(2, 300, 128) == 1                                    # never less than one query
    assert step_blocks(6, 0, 128) == 6                                      # an empty corpus counts as one chunk


def test_csr_rows_normalises_in_both_modes():
    from snx.retrieval import exclusion_csr, relevance_csr
    from snx.retrieval._common import csr_rows
    rows = [[5, 1, 5], [], [9, 0, 9, 3]]                                    # unsorted, duplicates, an empty row
    for got in (exclusion_csr(rows, 3, 10, "cpu"), relevance_csr(rows, 3, 10, "cpu"),
                csr_rows(rows, 3, 10, "cpu", "exclusion", True), csr_rows(rows, 3, 10, "cpu", "relevance", False)):
        ptr, docs = got
        assert ptr.tolist() == [0, 2, 2, 5] and docs.tolist() == [1, 5, 0, 3, 9]
        assert ptr.dtype == torch.long and docs.dtype == torch.int32
    # ids outside the corpus: kept in a relevance row (any int32, in numeric order), refused in an exclusion row
    out = [[12, -1, 3], [2 ** 31 - 1, -2 ** 31, 10]]
    ptr, docs = relevance_csr(out, 2, 10, "cpu")
    assert ptr.tolist() == [0, 3, 6] and docs.tolist() == [-1, 3, 12, -2 ** 31, 10, 2 ** 31 - 1]
    for bad in ([[12], []], [[-1], []], [[3], [10]]):
        with pytest.raises(ValueError, match=r"^exclusion rows: doc ids must lie in \[0, 10\)$"):
            exclusion_csr(bad, 2, 10, "cpu")
    with pytest.raises(ValueError, match=r"^relevance rows: doc ids must fit in int32$"):
        relevance_csr([[2 ** 31]], 1, 10, "cpu")
    with pytest.raises(ValueError, match=r"^relevance rows: doc ids must be ints$"):
        relevance_csr([[1.0]], 1, 10, "cpu")
    # a CSR pair whose first row is unsorted and repeats an id; int32 ptr
    pair = (torch.tensor([0, 3, 3, 4], dtype=torch.int32), torch.tensor([7, 2, 7, 0]))
    for f in (exclusion_csr, relevance_csr):
        ptr, docs = f(pair, 3, 10, "cpu")
        assert ptr.tolist() == [0, 2, 2, 3] and docs.tolist() == [2, 7, 0] and docs.dtype == torch.int32
    ptr, docs = relevance_csr((torch.tensor([0, 2]), torch.tensor([40, -3])), 1, 10, "cpu")
    assert ptr.tolist() == [0, 2] and docs.tolist() == [-3, 40]
    with pytest.raises(ValueError, match=r"^exclusion rows: doc ids must lie"):
        exclusion_csr((torch.tensor([0, 2]), torch.tensor([40, -3])), 1, 10, "cpu")
    for f, what in ((exclusion_csr, "exclusion"), (relevance_csr, "relevance")):
        with pytest.raises(ValueError, match=rf"^{what} rows: ptr must start at 0"):
            f((torch.tensor([0, 2, 1]), torch.tensor([1, 2])), 2, 10, "cpu")
        with pytest.raises(ValueError, match=rf"^{what} rows: a CSR pair needs int tensors ptr \[3\]"):
            f((torch.tensor([0, 2]), torch.tensor([1, 2])), 2, 10, "cpu")
        with pytest.raises(ValueError, match=rf"^{what} rows: 1 rows for 2 queries$"):
            f([[1]], 2, 10, "cpu")
        ptr, docs = f([], 0, 0, "cpu")                                      # no query, no corpus
        assert ptr.tolist() == [0] and docs.numel() == 0


def test_targets_validator_with_and_without_the_range_check():
    from snx.retrieval._common import check_targets
    cpu = torch.device("cpu")
    assert check_targets(None, 3, 10, cpu, "X.search") is None
    t = torch.tensor([9, 0, 4, 7])[::2]                                     # int64, not contiguous
    got = check_targets(t, 2, 10, cpu, "X.search")
    assert got.dtype == torch.int32 and got.is_contiguous() and got.tolist() == [9, 4]
    assert check_targets(torch.zeros(0, dtype=torch.int32), 0, 0, cpu, "X.search").numel() == 0
    for bad in (torch.tensor([1, 2, 3]), torch.tensor([1.0, 2.0]), torch.tensor([[1, 2]]), [1, 2],
                torch.tensor([1, 2], dtype=torch.int16)):
        for nd in (10, None):
            with pytest.raises(ValueError, match=r"^X\.search: targets must be an int tensor \[2\] on cpu$"):
                check_targets(bad, 2, nd, cpu, "X.search")
    with pytest.raises(ValueError, match=r"^X\.search: targets must be an int tensor"):
        check_targets(torch.tensor([1, 2]), 2, 10, torch.device("meta"), "X.search")     # another device
    for bad in (torch.tensor([1, 10]), torch.tensor([-1, 2])):
        with pytest.raises(ValueError, match=r"^SparseIndex\.rescore: targets must be doc ids in \[0, 10\)$"):
            check_targets(bad, 2, 10, cpu, "SparseIndex.rescore")
        assert check_targets(bad, 2, None, cpu, "fuse_ranked").tolist() == bad.tolist()   # nd=None: no range check
