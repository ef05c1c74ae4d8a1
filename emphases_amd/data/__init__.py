"""`emphases.data` of the reference: `emphases.data.preprocess` writes the
feature cache of whole datasets (`preprocess.datasets`); `Dataset`, `Sampler`
and `Loader` read it back for training, resident on the device (partitions
and downloads stay out of scope)."""
from . import preprocess  # noqa: F401
from .collate import collate  # noqa: F401
from .dataset import Dataset  # noqa: F401
from .loader import Loader  # noqa: F401
from .sampler import Sampler  # noqa: F401
