"""The optional ``idf:`` section of the training YAML (ref:docs/reference/hyperparameters.md "V26 IDF"): IDF-aware FLOPS
training and the inference-free ("doc-only") query mode.  A section of its own, not a field of ``V33Config`` -- the V33
dataclasses mirror the reference's and stay as they are; the V33 loader ignores the key.

    idf:
      idf_weights_path: outputs/idf_weights/idf      # .bin + .json of src.train.cli.compute_idf (or a .pt tensor)
      idf_alpha: 4.0
      beta: 0.3
      special_token_penalty: 100.0
      stopword_penalty: 15.0
      stopword_file: data/stopwords.txt               # one token per line, resolved through the tokenizer
      query_mode: idf                                 # "encoder" (default) or "idf" (doc-only)
      query_idf_path: null                            # the query table when it differs from idf_weights_path
"""
from dataclasses import dataclass, fields
from pathlib import Path
from typing import Optional

QUERY_MODES = ("encoder", "idf")
SMOOTHINGS = ("bm25", "standard", "smooth")


@dataclass
class IdfConfig:
    idf_weights_path: Optional[str] = None
    idf_smoothing: str = "bm25"
    idf_alpha: float = 4.0
    beta: float = 0.3
    special_token_penalty: float = 100.0
    stopword_penalty: float = 15.0
    stopword_file: Optional[str] = None
    query_mode: str = "encoder"
    query_idf_path: Optional[str] = None

    def __post_init__(self):
        if self.query_mode not in QUERY_MODES:
            raise ValueError(f"idf.query_mode must be one of {QUERY_MODES}, not {self.query_mode!r}")
        if self.idf_smoothing not in SMOOTHINGS:
            raise ValueError(f"idf.idf_smoothing must be one of {SMOOTHINGS}, not {self.idf_smoothing!r}")

    @property
    def enabled(self) -> bool:
        return self.idf_weights_path is not None

    @property
    def doc_only(self) -> bool:
        return self.query_mode == "idf"


def load_idf_config(raw: Optional[dict], idf_weights: Optional[str] = None,
                    query_mode: Optional[str] = None) -> Optional[IdfConfig]:
    """The ``idf:`` section of a parsed YAML document plus the CLI overrides (--idf-weights, --query-mode) -> IdfConfig,
    or None when neither is present: the trainer then builds SPLADELossV33 exactly as without this module."""
    section = (raw or {}).get("idf")
    if section is None and idf_weights is None and query_mode is None:
        return None
    section = dict(section or {})
    known = {f.name for f in fields(IdfConfig)}
    bad = sorted(set(section) - known)
    if bad:
        raise ValueError(f"idf: unknown keys {bad}; known: {sorted(known)}")
    cfg = IdfConfig(**section)
    if idf_weights is not None:
        cfg.idf_weights_path = idf_weights
    if query_mode is not None:
        cfg.query_mode = query_mode
        cfg.__post_init__()
    if not cfg.enabled:
        raise ValueError("idf: idf_weights_path (or --idf-weights) is required")
    return cfg


def read_stopwords(path) -> list:
    """One token per line; blank lines and lines starting with '#' are skipped."""
    out = []
    for line in Path(path).read_text(encoding="utf-8").splitlines():
        line = line.strip()
        if line and not line.startswith("#"):
            out.append(line)
    return out


def build_idf_loss(cfg: IdfConfig, loss_kwargs: dict, tokenizer, vocab_size: int):
    """IdfConfig -> SPLADELossIDF (on the CPU; the caller moves it).  The IDF table is padded with its maximum (an id the
    corpus never showed is as rare as the rarest) or cut to the model's vocabulary."""
    import numpy as np
    import torch

    from benchmark.encoders import allowed_token_mask, special_token_ids
    from snx.idf import load_idf, penalty_weights
    from src.model.losses import SPLADELossIDF

    def table(path):
        w, _ = load_idf(path)
        if w.shape[0] < vocab_size:
            w = np.concatenate([w, np.full(vocab_size - w.shape[0], w.max(), dtype=np.float32)])
        return w[:vocab_size]

    idf = table(cfg.idf_weights_path)
    special = sorted(i for i in special_token_ids(tokenizer) if 0 <= i < vocab_size)
    stop = []
    if cfg.stopword_file:
        unk = getattr(tokenizer, "unk_token_id", None)
        for tok in read_stopwords(cfg.stopword_file):
            for i in tokenizer.encode(tok, add_special_tokens=False):
                if i != unk and 0 <= i < vocab_size and i not in special:
                    stop.append(int(i))
    w = penalty_weights(idf, alpha=cfg.idf_alpha, special_ids=special, special_penalty=cfg.special_token_penalty,
                        stopword_ids=stop, stopword_penalty=cfg.stopword_penalty)
    query_idf = query_allowed = None
    if cfg.doc_only:
        query_idf = torch.from_numpy(table(cfg.query_idf_path or cfg.idf_weights_path).copy())
        known = min(vocab_size, int(getattr(tokenizer, "vocab_size", vocab_size)))
        lookup = list(tokenizer.convert_ids_to_tokens(list(range(known))))
        query_allowed = allowed_token_mask(lookup, set(special), vocab_size)
    return SPLADELossIDF(penalty_weights=w, beta=cfg.beta, query_idf=query_idf, query_allowed=query_allowed, **loss_kwargs)
