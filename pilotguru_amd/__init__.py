"""pilotguru_amd -- MI355X-native ORB front end for pilotguru's optical_trajectories.

Only what the hot path needs: csrc/ (HIP kernels + C ABI, built into libpgorb.so),
the host-side mirror of the reference's ORBextractor / ORBmatcher interface (orb.py),
and the synthetic ride generator used by tests and bench (synth.py).
"""
from .orb import KEYPOINT_DTYPE, DeviceFrameStream, Frame, FrameStream, MapPoints, ORBextractor, ORBmatcher  # noqa: F401
from .orb import KF_POSE_DTYPE, NEW_MAP_POINT_DTYPE, LocalMapping, kf_pose  # noqa: F401
from .orb import MAP_POINT_DTYPE, MapPointTable, SIM3_DTYPE, sim3_pose, sim3_record  # noqa: F401
from .orb import MP_BOTH, MP_DESCRIPTOR, MP_LIMIT, MP_MAX_OBS, MP_NORMAL_DEPTH  # noqa: F401
from .orb import PO_FEW, PO_INFO, PO_NONFINITE, Optimizer  # noqa: F401
from .orb import OS3_FEW, OS3_INFO, OS3_NONFINITE  # noqa: F401
from .orb import (LBA_INFO, LBA_LIMIT, LBA_MAX_EDGES, LBA_MAX_FIXED_KF, LBA_MAX_LOCAL_KF, LBA_MAX_POINTS, LBA_NONFINITE,  # noqa: F401
                  LBA_NOTHING, LBA_ROLE_FIXED, LBA_ROLE_LOCAL, LBA_ROLE_NONE)
from .orb import (EG_EDGE_DTYPE, EG_INFO, EG_LIMIT, EG_MAX_EDGES, EG_MAX_ENVELOPE_BLOCKS, EG_MAX_KF, EG_NONFINITE, EG_NOTHING,  # noqa: F401
                  SIM3D_DTYPE)
from .orb import (GBA_INFO, GBA_LIMIT, GBA_MAX_EDGES, GBA_MAX_ENVELOPE_BLOCKS, GBA_MAX_KF, GBA_MAX_POINTS, GBA_NONFINITE,  # noqa: F401
                  GBA_NOTHING)
from .orb import S3_FEW, S3_FOUND, S3_INFO, S3_NO_MORE, SIM3_ESTIMATE_DTYPE, SIM3_MAX_ITERATIONS, SIM3_PARAMS_DTYPE, Sim3Solver  # noqa: F401
from .orb import (PNP_FEW, PNP_FOUND, PNP_HYPOTHESIS_DTYPE, PNP_INFO, PNP_MAX_WINDOW, PNP_NO_MORE, PNP_PARAMS_DTYPE, PNP_REFINED,  # noqa: F401
                  PnPsolver)
from .orb import (INIT_AMBIGUOUS, INIT_DEGENERATE_H, INIT_FEW, INIT_FEW_GOOD, INIT_FINFO, INIT_HYPOTHESIS_DTYPE, INIT_INFO,  # noqa: F401
                  INIT_LOW_PARALLAX, INIT_MAX_ITERATIONS, INIT_MODEL_F, INIT_MODEL_H, INIT_NO_MODEL, INIT_OK, INIT_PARAMS_DTYPE, Initializer)
from .orb import (COVIS_EMPTY, COVIS_FALLBACK, COVIS_INFO, COVIS_LIMIT, COVIS_MAX_CONN, COVIS_MAX_KF, COVIS_PARENT_SET,  # noqa: F401
                  COVIS_RESORTED, COVIS_UPDATED, LOCALMAP_LIMIT, LOCALMAP_NO_VOTES, CovisibilityGraph, Tracking)
from .orb import (CULL_INFO, CULL_KF_CULLED, CULL_KF_ID0, CULL_KF_KEEP, CULL_KF_NONE, CULL_KF_TO_BE_ERASED, CULL_KF_WAS_BAD, CULL_LIMIT,  # noqa: F401
                  CULL_MP_AGED, CULL_MP_FEW_OBS, CULL_MP_FOUND_RATIO, CULL_MP_KEEP, CULL_MP_NONE, CULL_MP_WAS_BAD, CULL_ROW_CLEARED,
                  CULL_ROW_ERASED, CULL_ROW_REPARENTED, compact_observations)
from .orb import LC_BAD_INDEX, LC_INFO, LC_OVER_OBS, MU_INFO, LoopClosing  # noqa: F401
from .orb import (TCP_INFO, TRACK_BAD_INDEX, TRACK_FULL, TRACK_MAX, TRACK_MOTION_MODEL, TRACK_NO_LAST, TRACK_NO_VELOCITY,  # noqa: F401
                  TRACK_REFERENCE_KF, TRACK_STATE_DTYPE, TRAJ_BAD_TIME, TRAJ_BROKEN, TRAJ_INFO, TRAJ_MAX_RECORDS, TRAJ_NO_ORIGIN,
                  TRAJECTORY_RECORD_DTYPE, System)
from .orb import (DECIDE_INFO, DECIDE_LOCAL_MAP, DECIDE_MOTION_MODEL, DECIDE_REFERENCE_KF, DECIDE_WRONG_INIT, DEPTH_EMPTY, DEPTH_MAX_LIST,  # noqa: F401
                  DEPTH_NAN, TRACK_COUNTERS_DTYPE)
from .map_edit import (EDIT_ADD, EDIT_ALREADY, EDIT_APPLIED, EDIT_BAD_INDEX, EDIT_ERASE, EDIT_INFO, EDIT_LIMIT, EDIT_MAX_BAG,  # noqa: F401
                       EDIT_MAX_EDITS, EDIT_MAX_LIST, EDIT_NOP, EDIT_NOT_OBSERVED, EDIT_REPLACE, EDIT_SELF, EDIT_SET_REF, EDIT_TOUCH_CHANGED,
                       EDIT_TOUCH_STALE, EDIT_TOUCH_SURVIVOR, EDIT_WENT_BAD, MAP_EDIT_DTYPE, apply_map_edits, map_edits,
                       map_edits_from_fuse, map_edits_from_keyframe, map_edits_from_lba_erase, map_edits_from_loop_matches,
                       observation_ids)
from .place import KeyFrameDatabase  # noqa: F401
