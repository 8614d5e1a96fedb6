"""Mirror of the reference's ``src.preprocessing`` for the one part that runs on the GPU here: the cleaners'
deduplicators (``src.preprocessing.cleaners``).  The rest of the reference's preprocessing (converters, the Korean text
cleaner, the pipeline) is host text work and is not part of this project."""
