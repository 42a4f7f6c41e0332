from .carla_seg import CARLA_Seg, collate_padded  # noqa: F401
