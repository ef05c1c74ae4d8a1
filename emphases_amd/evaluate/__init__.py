"""`emphases.evaluate`: `datasets` (the dataset evaluation of
`emphases/evaluate/core.py`), `Metrics` and `metrics` (the word-level metrics
of `emphases_amd.metrics`)."""
from .core import datasets  # noqa: F401
from .. import metrics  # noqa: F401
from ..metrics import Metrics  # noqa: F401
