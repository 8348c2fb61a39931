"""linemod_pose_estimation_amd -- MI355X-native LINEMOD template matching behind the reference's
rgbdDetector::linemod_detection / cv::linemod::Detector::match call surface.

Only what the hot path needs lives here: csrc/ (HIP kernels + C ABI -> liblmx.so), the host-side mirror of the
reference interface (detector.py; NativeBank.train_mesh / render_views: the trainer from a mesh; DepthTemplates: the depth check of matches and, after enable_normals, the normal term), the bank container (bank.py), the synthetic bank/scene generator the tests
and bench use (synth.py) and the template-shard helper for multi-GPU runs (dist.py).
"""
from .bank import TemplateBank  # noqa: F401
from .detector import Detector, NativeBank, PinnedArena, linemod_detection, merge_raw, render_views, MATCH_DTYPE, RAW_MATCH_DTYPE  # noqa: F401
from .detector import DepthTemplates, DEPTH_DIFF_DTYPE, cluster_matches_scored, depth_values  # noqa: F401
from .detector import NORMAL_DIFF_DTYPE, normal_values, normal_angle_table  # noqa: F401
from .detector import cluster_matches_classes  # noqa: F401
from .detector import POSE_REFINE_DTYPE, compose_pose, cluster_leaders  # noqa: F401
from .detector import POSE_VERIFY_DTYPE, keep_verified  # noqa: F401
from .detector import device_images  # noqa: F401
from .detector import ExportedMatches, export_layout  # noqa: F401
from .detector import ExportedClusters, export_clusters_layout  # noqa: F401
from .detector import ExportedPoses, pose_chain_layout  # noqa: F401
from .detector import RoughModel, ExportedRoughPoses, ROUGH_POSE_DTYPE, rough_pose_layout, rough_trace_min  # noqa: F401
