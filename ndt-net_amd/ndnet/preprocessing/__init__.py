from .fps import farthest_point_sample, fps_downsample  # noqa: F401
from .nearest import nearest_sample  # noqa: F401
from .sample import RandomSample, gather_samples, random_sample  # noqa: F401
from .ndt_legacy import NDT_Sampler  # noqa: F401
from .ndtnet_preprocessing import ndt_preprocessing  # noqa: F401
