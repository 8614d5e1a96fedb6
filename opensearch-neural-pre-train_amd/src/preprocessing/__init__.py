"""Mirror of the reference's ``src.preprocessing`` for the parts that run on the GPU here: the cleaners' deduplicators
(``src.preprocessing.cleaners``), the dense hard-negative miner (``src.preprocessing.miners``) and the MLM corpus
preparation (``src.preprocessing.mlm_data``: the reference's ``scripts/prepare_korean_mlm_data.py`` -- paragraph split,
length and Hangul filter, SHA-256 dedup -- because its output is the input of ``src.train.cli.pretrain_mlm``).  The rest
of the reference's preprocessing (converters, the regex-based ``KoreanTextCleaner``, ``pipeline.py``) is host text work
and is not part of this project."""
