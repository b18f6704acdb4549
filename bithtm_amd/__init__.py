"""bithtm_amd -- MI355X-native per-timestep hot path of bitHTM (Spatial Pooler + Temporal
Memory) behind the reference's Python class surface (bithtm/__init__.py:4-6).

    from bithtm_amd import HierarchicalTemporalMemory      # instead of: from bithtm import ...

The classes are host-side shells around hand-written HIP kernels for gfx950 reached through a
C ABI (include/bithtm_hip.h, libbithtm_hip.so).  There is no CPU fallback: importing the
engine without the built library raises ImportError."""

from . import classifier, encoders, likelihood, networks
from .anomaly import AnomalyLikelihood  # noqa: F401
from .sdr_classifier import SDRClassifier, SDRClassifierBank  # noqa: F401
from .knn_classifier import KNNClassifier, KNNClassifierBank  # noqa: F401
from .encoders import CategoryField, CoordinateField, HashedField, ScalarEncoder, ScalarField, date_fields, date_values, geo_values  # noqa: F401
from .networks import InferenceView, flip_noise, noise_threshold  # noqa: F401
from .engine import CapacityError, HtmError  # noqa: F401
from .group import GroupTick, ModelGroup  # noqa: F401
from .stack import RegionStack  # noqa: F401
from .group_stack import GroupStack  # noqa: F401
from .pooling import PoolingLink  # noqa: F401
from .projections import DenseProjection, PredictiveProjection  # noqa: F401
from .regularizations import ExponentialBoosting, GlobalInhibition  # noqa: F401

SpatialPooler = networks.SpatialPooler
TemporalMemory = networks.TemporalMemory
HierarchicalTemporalMemory = networks.HierarchicalTemporalMemory
RunRecord = networks.RunRecord
SPRunRecord = networks.SPRunRecord
