"""`emphases.data.preprocess`: `from_audio` and the `mels` / `loudness`
modules on the HIP front-end, and the feature cache of whole datasets
(`datasets`, `from_files_to_files`, `python -m emphases_amd.data.preprocess`)
in ragged batches of files.  Loaders and partitions stay out of scope
(DESIGN.md section 10)."""
from .core import from_audio  # noqa: F401
from .core import datasets, from_files_to_files  # noqa: F401
from . import mels  # noqa: F401
from . import loudness  # noqa: F401
