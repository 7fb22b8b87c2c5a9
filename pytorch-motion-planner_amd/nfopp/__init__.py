"""nfopp -- MI355X-native inner loop of the Neural Field Optimal Path Planner.

Host-side mirror of the reference's planner interface over libnfopp_hip.so (C ABI: include/nfopp_hip.h).
"""
from ._lib import LIB_PATH, NUM_PATH_STATS, PATH_STAT_NAMES, NfoppError, load as load_library
from .batch import BatchPlanner, OnfFitter, shard_range, straight_line_init
from .engine import TrajectoryEngine, TrajectoryHyper, band_of, inverse_hessian
from .distance_field import DistanceField
from .heading_field import HeadingDistanceField
from .moving import MovingObstacles
from .conflicts import (CONFLICT_BAD_TRACK, CONFLICT_COUNT, CONFLICT_FIRST_PARTNER, CONFLICT_FIRST_TIME, CONFLICT_MIN_GAP,
                        CONFLICT_MIN_PARTNER, CONFLICT_MIN_TIME, CONFLICT_NO_PARTNER, CONFLICT_STATUS, BoxTrackConflicts,
                        TrackConflicts, box_track_conflicts, constant_velocity_tracks, track_conflicts, track_headings)
from .schedule import (SCHEDULE_BAD_TRACK, SCHEDULE_MAX_DELAY, SCHEDULE_NOT_ORDERED, SCHEDULE_OK, SCHEDULE_UNRESOLVED, FleetMasks,
                       FleetSchedule, delay_tracks, fleet_box_shift_masks, fleet_shift_masks, schedule_box_delays, schedule_delays)
from .spacetime import (SPACETIME_BAD_CELL, SPACETIME_DIRECTIONS, SPACETIME_NOT_ORDERED, SPACETIME_OK, SPACETIME_UNREACHED,
                        SpaceTimePlan, SpaceTimeReservation, spacetime_plan)
from .factory import DEFAULT_PARAMETERS, PlannerFactory, UniversalFactory
from .grid_search import (AstarTrajectoryInitializer, OccupancyGrid, distance_fields, grid_search_init, grid_search_paths,
                          margin_cells2, seed_polylines, seed_trajectories, shorten_paths)
from .host_utils import (AttributeDict, CircleCollisionChecker,
                         CircleDirectedCollisionChecker, CollisionChecker, Position2, RectangleCollisionChecker,
                         TrajectoryInitializer)
from .lattice import (GearLattice, LatticeGrid, heading_index, lattice_fields, lattice_gear_fields, lattice_gear_search_init,
                      lattice_gear_search_paths, lattice_search_init, lattice_search_paths, seed_lattice_trajectories)
from .learning import BatchSampler, DeviceCircleChecker, DeviceGridChecker, DeviceGridMap, DeviceRectangleChecker
from .onf_model import ONF
from .path_tools import PathPostprocessor, init_trajectories
from .planner import ConstrainedNERFOptPlanner, ContinuousPlanner, NERFOptPlanner
from .time_profile import (TIME_GOAL_UNREACHABLE, TIME_OUT_OF_RANGE, TIME_SLOT_S, TIME_SLOT_T, TIME_SLOT_V, TIME_SLOT_V_PEAK,
                           TIME_START_TOO_FAST, TIME_SUMMARY_LENGTH, TIME_SUMMARY_STATUS, TIME_SUMMARY_STOPS,
                           TIME_SUMMARY_TIME, MotionLimits, TimedPaths, time_parametrize)

# slots of BatchPlanner.path_stats' [B, 8] result (NFOPP_PATH_STAT_* of include/nfopp_hip.h)
(PATH_STAT_LENGTH, PATH_STAT_MAX_CURVATURE, PATH_STAT_CURVATURE_AT, PATH_STAT_CUSPS, PATH_STAT_REVERSALS,
 PATH_STAT_MIN_CLEARANCE, PATH_STAT_CLEARANCE_AT, PATH_STAT_MEAN_CLEARANCE) = range(NUM_PATH_STATS)

__all__ = [
    "BatchPlanner", "BatchSampler", "DistanceField", "HeadingDistanceField", "MovingObstacles", "DeviceCircleChecker", "DeviceGridChecker", "DeviceGridMap", "DeviceRectangleChecker", "OnfFitter", "shard_range", "straight_line_init", "LIB_PATH", "NfoppError", "load_library", "TrajectoryEngine", "TrajectoryHyper", "band_of", "inverse_hessian",
    "DEFAULT_PARAMETERS", "PlannerFactory", "UniversalFactory", "AstarTrajectoryInitializer", "AttributeDict",
    "CircleCollisionChecker", "CircleDirectedCollisionChecker", "CollisionChecker", "Position2",
    "RectangleCollisionChecker", "TrajectoryInitializer", "ONF", "ConstrainedNERFOptPlanner", "ContinuousPlanner",
    "NERFOptPlanner", "PathPostprocessor", "init_trajectories", "OccupancyGrid", "grid_search_init", "grid_search_paths",
    "distance_fields", "seed_trajectories", "seed_polylines", "shorten_paths", "margin_cells2", "NUM_PATH_STATS", "PATH_STAT_NAMES", "PATH_STAT_LENGTH",
    "PATH_STAT_MAX_CURVATURE", "PATH_STAT_CURVATURE_AT", "PATH_STAT_CUSPS", "PATH_STAT_REVERSALS",
    "PATH_STAT_MIN_CLEARANCE", "PATH_STAT_CLEARANCE_AT", "PATH_STAT_MEAN_CLEARANCE",
    "MotionLimits", "TimedPaths", "time_parametrize", "TIME_SLOT_S", "TIME_SLOT_T", "TIME_SLOT_V", "TIME_SLOT_V_PEAK",
    "TIME_SUMMARY_TIME", "TIME_SUMMARY_LENGTH", "TIME_SUMMARY_STOPS", "TIME_SUMMARY_STATUS", "TIME_START_TOO_FAST",
    "TIME_GOAL_UNREACHABLE", "TIME_OUT_OF_RANGE",
    "TrackConflicts", "track_conflicts", "constant_velocity_tracks", "CONFLICT_MIN_GAP", "CONFLICT_MIN_PARTNER",
    "CONFLICT_MIN_TIME", "CONFLICT_FIRST_TIME", "CONFLICT_FIRST_PARTNER", "CONFLICT_COUNT", "CONFLICT_STATUS",
    "CONFLICT_BAD_TRACK", "CONFLICT_NO_PARTNER", "BoxTrackConflicts", "box_track_conflicts", "track_headings",
    "FleetMasks", "FleetSchedule", "fleet_shift_masks", "fleet_box_shift_masks", "schedule_delays", "schedule_box_delays", "delay_tracks", "SCHEDULE_OK", "SCHEDULE_BAD_TRACK",
    "SCHEDULE_UNRESOLVED", "SCHEDULE_NOT_ORDERED", "SCHEDULE_MAX_DELAY",
    "SpaceTimePlan", "SpaceTimeReservation", "spacetime_plan", "SPACETIME_OK", "SPACETIME_BAD_CELL", "SPACETIME_UNREACHED",
    "SPACETIME_NOT_ORDERED", "SPACETIME_DIRECTIONS",
    "LatticeGrid", "heading_index", "lattice_fields", "lattice_search_paths", "lattice_search_init",
    "GearLattice", "lattice_gear_fields", "lattice_gear_search_paths", "lattice_gear_search_init", "seed_lattice_trajectories",
]
