"""Mirror of the reference's ``src.preprocessing`` for the parts that run on the GPU here: the cleaners' deduplicators
(``src.preprocessing.cleaners``) and the dense hard-negative miner (``src.preprocessing.miners``).  The rest of the
reference's preprocessing (converters, the Korean text cleaner, the pipeline) is host text work and is not part of this
project."""
