"""simple_knn._C of upstream 3DGS on gaussreg_amd.scene_init (csrc/scene_init.hip)."""
from gaussreg_amd.scene_init import mean_knn_dist2


def distCUDA2(points):
    return mean_knn_dist2(points, 3)
