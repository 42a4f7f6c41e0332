from .carla_seg import CARLA_Seg, collate_packed, collate_padded  # noqa: F401
