"""Plan a path to a named object on a saved VLMap: name -> goal cell -> path.  Counterpart of the reference's HabitatLanguageRobot
setup_scene + move_to (robot/habitat_lang_robot.py:88-104, 432-461) without the simulator.

    python -m avlmaps_amd.apps.plan_path --data-dir <scene> --query sofa --start ROW COL [--text-model clip|hash]
                                        [--area NAME]... [--sound NAME]... [--image PNG] [--goal-2d [--travel [--travel-from-start] [--sound-travel]]]
                                        [--tour NAME,NAME,... [--tour-closed]]
                                        [--customize-obstacles [--potential-obstacles a,b,c --obstacles a,b]
                                         [--dilate-iter N] [--gaussian-sigma S]]
                                        [--relation left|right|between|north|south|east|west|face --heading DEG [--query-b NAME]]
                                        [--nearest euclid|path] [--known-free] [--goal object|frontier|nbv] [--render PNG]
                                        [--goal nbv [--view-range METRES] [--nbv-count K] [--nbv-conservative]]
                                        [--view [--view-range METRES] [--view-fraction F]]
                                        [--room NAME|ID [--door-width M] [--room-names a,b,c]]
                                        [--planner visgraph|cost [--robot-radius M] [--inflation-radius M] [--cost-scaling K]
                                         [--avoid NAME[:RADIUS[:PENALTY]]]...]

Loads <scene>/vlmap/vlmaps.h5df (with --text-model hash a missing map is first created with the model-free feature stand-in, as
apps.create_map --features hash does), builds the obstacle map (Map.generate_obstacle_map), takes the goal from
Map.get_nearest_pos, plans with Navigator on the GPU and prints one JSON line: the query, the start, the goal and the path, all
in full-map (row, col) cells.

With --area, --sound or --image the goal is cross-modal (habitat_lang_robot.py:377-430): the cell of
AVLMap.index_goal(obj=--query, area=.., sound=.., img=..), handed to Navigator.plan_to as it is -- a goal voxel is an occupied
voxel, and the planner snaps a goal on an obstacle cell to the nearest free cell.  The JSON line then also has "goal_voxel",
"goal_value" (0.0: the modalities do not overlap anywhere) and "goal_cell", the voxel's own cell; "goal" is that cell clamped into
the cropped obstacle map, which differs only when the voxel's height is outside --h-min / --h-max and nothing in the band reaches
that far.

With --goal-2d the goal is taken on the planner's own grid instead: the cell of AVLMap.index_goal_2d(obj=--query, area=..,
sound=..), the first maximum of the product of the 2-D distribution maps over the obstacle crop (habitat_lang_robot.py:357-375,
419-425).  The JSON line then has "goal_value" and "goal_cell"; the cell lies inside the crop, so "goal" equals it.  --image has no
2-D map and is rejected.  With --goal-2d --travel the object factor decays with the travel distance on the obstacle crop instead
of the straight line (AVLMap.index_goal_2d_travel, csrc/avl_travel.hip): the goal cell is near the object by the way the robot has
to walk, not through a wall; --travel-from-start multiplies in the travel decay from --start, which prefers the nearest of
several objects by that way.  Area and sound factors stay Euclidean, unless --sound-travel asks for the sound factors around walls
as well (AVLMap.index_sound_2d_travel, csrc/avl_travel_many.hip: one travel field per sound segment, in batches).

With --tour NAME,NAME,... (1 to 10 objects, no --query) the robot visits all of them in the best order (VLMap.plan_object_tour: one
batch of travel fields over the start and the objects' cells, the set-to-set distances, an exact Held-Karp on them); --tour-closed
comes back to --start.  The JSON line has "tour" (the names in visiting order), "skipped" (the names no walk from --start reaches),
"matrix_length" and "driven_length" in cells, and "legs", the cells of every leg's walk.  It plans no single path: the flags that
choose another goal or planner, --known-free and --render are rejected.

With --customize-obstacles the path is planned on Map.get_customized_obstacle_cropped() as upstream's robot does
(habitat_lang_robot.py:89-104): VLMap.customize_obstacle_map keeps only the obstacles whose class is one of --obstacles among
--potential-obstacles and smooths the map (Map._dilate_map with --dilate-iter and --gaussian-sigma).  The four values default to
the map config's (config/map_config/vlmaps.yaml:14-15 upstream).

With --nearest path the goal is the --query object's contour point with the shortest travel distance from --start
(Map.get_nearest_reachable_pos: one shortest-path tree and one launch over all candidates) instead of the nearest as the crow
flies, which may lie behind a wall.

With --relation the goal is one of the robot's spatial-relation goals (Map.get_left_pos, get_right_pos, get_pos_in_between,
get_north_pos / get_south_pos / get_east_pos / get_west_pos; map.py:366-485 upstream) for a robot at --start heading --heading
degrees (0 = towards smaller rows, clockwise positive).  `between` takes the second object from --query-b.  The JSON line then has
"relation", "heading" and "goal_cell", the method's own result; "goal" is that point clamped into the cropped obstacle map.
`face` plans nothing: it prints the angle to turn right to face the nearest --query object (Map.get_delta_angle_to) as
"turn_right_deg".  A relation with nothing in front of the robot ends with a message and exit status 1.

With --known-free the path is planned on Map.get_known_free_cropped(): the obstacle map (the customised one with
--customize-obstacles) AND-ed with the explored map, so that the plan stays in space a camera has seen (needs
<scene>/vlmap/explored.npz, apps.create_map --explored).  With --goal frontier the goal is not an object at all but where to look
next: the frontier of the explored area with the shortest travel distance from --start (Map.get_frontiers,
Navigator.plan_to_nearest_frontier), planned on the known-free map; --query is not needed, and the JSON line has "frontiers", the
number of frontier islands, and "frontier_cells", the size of the chosen one.

With --goal nbv the goal is the next best view (Map.get_next_best_view; csrc/avl_viewshed.hip): among the known-free
cells on a lattice and the frontier centres that the robot can reach, those from which at least half as many unknown cells would
become visible within --view-range metres (default 3) as from the best one, and of these the one with the shortest travel distance
from --start.  The path is planned on the known-free map.  The JSON line has "goal_kind": "nbv", "gain" (the unknown cells the goal
would see), "heading_octant" (the first of the two neighbouring 45-degree sectors of atan2(d_row, d_col) that hold the most of
them) and "views", the tour of Map.plan_exploration with --nbv-count K views (default 1): [{"goal", "heading_octant", "gain"}, ...],
each chosen on the map as it would be known after the views before it.  --nbv-conservative lets unknown cells block the view, so
that only the first layer of unknown cells behind known space counts.  --render tints the cells the first view would see and marks
every view of the tour.  A fully explored map ends with a message and exit status 1.  Sight lines are 2-D, in the explored map's
height band; the robot's field of view is not modelled beyond the sector sums.

With --view the goal is not the object's contour point but a cell the object can be SEEN from (Map.get_viewpoints: 3-D sight lines
from a camera at the map config's camera height to the object's voxels, through the voxel map; csrc/avl_sight.hip): among the free
cells of the map the path is planned on (the customised one with --customize-obstacles, the known-free one with --known-free)
within --view-range metres (default 3) of the object that see at least --view-fraction (default 0.5) of what the best cell sees,
the one nearest to --start as the crow flies, or by travel distance with --nearest path (Map.get_viewpoint_pos).  The JSON line
then has "goal_kind": "viewpoint", "visible" (the object's voxels seen from the goal), "view_targets" (the voxels tested) and
"view_cells" (the cells that see any); --render tints those cells.  The robot's heading and field of view are not modelled.  An
object that no free cell in range sees ends with a message and exit status 1.

With --room the goal is a room, not an object: the centre of room ID of Map.get_rooms (on the customised map with
--customize-obstacles, which is what keeps furniture from splitting rooms), the room's cell farthest from every obstacle.  A NAME
is resolved through AVLMap.name_rooms over --room-names (default: the name alone): among the rooms that get the name, the one with
the highest mean frame score.  --door-width (default 0.9 m) is the widest opening that still separates rooms.  --query is not
needed; the JSON line has "goal_kind": "room", "room", "rooms" and "route", the rooms from --start's to the goal's through the
fewest doors (null when --start lies in no room or the two are not connected).

With --planner cost the path to the goal is not the Navigator's visibility-graph path, which is shortest and so touches every
corner it turns around, but the cheapest 8-connected walk on a costmap of the obstacle crop (Map.get_costmap, Map.plan_cost_path;
DESIGN.md 4.29, csrc/avl_costfield.hip): cells closer to an obstacle than --robot-radius (default 0.15 m) are impassable, the price
then decays with the clearance at --cost-scaling per metre (default 5) out to --inflation-radius (default 0.5 m), and every
--avoid NAME[:RADIUS[:PENALTY]] (repeatable; defaults 0.3 m and 200) adds a penalty on and around the cells of that category, which
joins the category list.  The goal is chosen as without the flag; goals that the Navigator itself chooses among several (--goal
frontier or nbv, --view, --nearest path) are not offered.  The path lists the start's cell, the cells where the direction changes
and the goal's cell; the JSON line gains "planner", "path_cost" (the summed price of the cells entered, diagonal steps times
sqrt(2), counted from the goal) and "min_clearance_m" (the smallest distance from a cell of the walk to an obstacle cell; null on a
map without obstacles).  The default, --planner visgraph, is the behaviour described above, unchanged.

With --render the plan is also drawn: the top-down colour map of the obstacle crop (Map.generate_rgb_topdown_map) with the
obstacle cells the planner used darkened, the path as a polyline, the start in green and the goal in red, as a PNG.  The JSON line
then has "render", the file.  With --planner cost the costmap lies under the path: the dearer a cell the redder, free cells that
the costmap makes impassable dark red."""
from __future__ import annotations

import argparse
import json


RELATIONS = ("left", "right", "between", "north", "south", "east", "west", "face")


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--data-dir", required=True)
    ap.add_argument("--query", default=None, help="the object to go to (not needed with --goal frontier)")
    ap.add_argument("--start", type=float, nargs=2, required=True, metavar=("ROW", "COL"), help="full-map cell of the robot")
    ap.add_argument("--config", default=None)
    ap.add_argument("--text-model", choices=["clip", "hash"], default="clip",
                    help="clip = OpenAI CLIP on PyTorch-ROCm (as upstream); hash = model-free stand-ins for smoke runs")
    ap.add_argument("--categories", default=None, help="comma separated category list of get_pos (default: the query and 'other')")
    ap.add_argument("--h-min", type=float, default=0.0)
    ap.add_argument("--h-max", type=float, default=1.5)
    ap.add_argument("--area", action="append", default=[], help="cross-modal goal: an area name (repeatable)")
    ap.add_argument("--sound", action="append", default=[], help="cross-modal goal: a sound name (repeatable)")
    ap.add_argument("--image", default=None, help="cross-modal goal: a query image (PNG)")
    ap.add_argument("--image-pose", type=int, default=0, help="row of poses.txt the model-free localiser places the image at")
    ap.add_argument("--goal-2d", action="store_true",
                    help="take the goal from the 2-D distribution maps over the obstacle crop (AVLMap.index_goal_2d)")
    ap.add_argument("--travel", action="store_true",
                    help="with --goal-2d: object factors decay with the travel distance around walls (AVLMap.index_goal_2d_travel)")
    ap.add_argument("--travel-from-start", action="store_true",
                    help="with --goal-2d --travel: one more factor, the travel decay from --start")
    ap.add_argument("--sound-travel", action="store_true",
                    help="with --goal-2d --travel and --sound: the sound factors decay around walls too (AVLMap.index_sound_2d_travel)")
    ap.add_argument("--tour", default=None, metavar="NAME,NAME,...",
                    help="visit these objects in the best order (VLMap.plan_object_tour): prints the order, the skipped goals and the legs")
    ap.add_argument("--tour-closed", action="store_true", help="with --tour: come back to --start at the end")
    ap.add_argument("--customize-obstacles", action="store_true",
                    help="plan on the customised obstacle map (VLMap.customize_obstacle_map) instead of the raw one")
    ap.add_argument("--potential-obstacles", default=None, help="comma separated class list the voxels are scored against")
    ap.add_argument("--obstacles", default=None, help="comma separated classes (of --potential-obstacles) that stay obstacles")
    ap.add_argument("--dilate-iter", type=int, default=None)
    ap.add_argument("--gaussian-sigma", type=float, default=None)
    ap.add_argument("--relation", choices=RELATIONS, default=None, help="take the goal from a spatial relation to --query")
    ap.add_argument("--heading", type=float, default=None, metavar="DEG", help="the robot's heading for --relation (0 = up, clockwise)")
    ap.add_argument("--query-b", default=None, metavar="NAME", help="the second object of --relation between")
    ap.add_argument("--nearest", choices=["euclid", "path"], default="euclid",
                    help="which --query object is the goal: euclid = the nearest as the crow flies (Map.get_nearest_pos); "
                         "path = the one with the shortest travel distance (Map.get_nearest_reachable_pos)")
    ap.add_argument("--known-free", action="store_true", help="plan on the obstacle map AND-ed with the explored map (Map.get_known_free_cropped)")
    ap.add_argument("--goal", choices=["object", "frontier", "nbv"], default="object",
                    help="object = go to --query (default); frontier = go to the nearest frontier of the explored area; "
                         "nbv = go to the next best view (Map.get_next_best_view)")
    ap.add_argument("--render", default=None, metavar="PNG", help="draw the crop, its obstacles, the path, start and goal")
    ap.add_argument("--view", action="store_true", help="go to a cell --query can be seen from (Map.get_viewpoint_pos), not to its contour")
    ap.add_argument("--view-range", type=float, default=None, metavar="METRES", help="how far from the object a viewpoint may be, or with --goal nbv how far the robot sees (default 3.0)")
    ap.add_argument("--view-fraction", type=float, default=None, metavar="F",
                    help="a viewpoint sees at least this fraction of what the best cell sees (default 0.5)")
    ap.add_argument("--nbv-count", type=int, default=None, metavar="K", help="--goal nbv: the views of the greedy tour (default 1)")
    ap.add_argument("--nbv-conservative", action="store_true", help="--goal nbv: unknown cells block the view")
    ap.add_argument("--room", default=None, metavar="NAME|ID", help="go to the centre of a room (Map.get_rooms): its id, or a name for AVLMap.name_rooms")
    ap.add_argument("--door-width", type=float, default=None, metavar="M", help="--room: openings up to M metres separate rooms (default 0.9)")
    ap.add_argument("--room-names", default=None, help="--room NAME: the comma separated names the rooms are named from (default: NAME alone)")
    ap.add_argument("--planner", choices=["visgraph", "cost"], default="visgraph",
                    help="visgraph = the Navigator's shortest visibility-graph path (default); cost = the cheapest walk on a costmap (Map.plan_cost_path)")
    ap.add_argument("--robot-radius", type=float, default=None, metavar="M", help="--planner cost: cells closer to an obstacle are impassable (default 0.15)")
    ap.add_argument("--inflation-radius", type=float, default=None, metavar="M", help="--planner cost: how far from an obstacle cells cost extra (default 0.5)")
    ap.add_argument("--cost-scaling", type=float, default=None, metavar="K", help="--planner cost: the decay of the inflation per metre (default 5.0)")
    ap.add_argument("--avoid", action="append", default=[], metavar="NAME[:RADIUS[:PENALTY]]",
                    help="--planner cost: keep off a category's cells: PENALTY (default 200) on them, falling to 0 at RADIUS metres (default 0.3); repeatable")
    args = ap.parse_args(argv)
    if args.tour is not None:
        args.tour = [c.strip() for c in args.tour.split(",") if c.strip()]
        if not 1 <= len(args.tour) <= 10:
            ap.error("--tour takes 1 to 10 comma separated object names")
        if (args.query is not None or args.goal != "object" or args.relation is not None or args.area or args.sound or args.image
                or args.goal_2d or args.view or args.nearest == "path" or args.room is not None or args.planner == "cost" or args.render
                or args.known_free):
            ap.error("--tour orders its own goals: no --query, --goal frontier or nbv, --relation, --area, --sound, --image, --goal-2d, "
                     "--view, --nearest path, --room, --planner cost, --known-free or --render")
    elif args.tour_closed:
        ap.error("--tour-closed belongs to --tour")
    if args.planner != "cost":
        if args.avoid or any(v is not None for v in (args.robot_radius, args.inflation_radius, args.cost_scaling)):
            ap.error("--avoid, --robot-radius, --inflation-radius and --cost-scaling belong to --planner cost")
    else:
        if args.goal != "object" or args.view or args.nearest == "path" or args.relation == "face":
            ap.error("--planner cost plans to one given goal: no --goal frontier or nbv, --view, --nearest path or --relation face")
        if args.avoid and args.room is not None:
            ap.error("--avoid names categories of an object goal's list: not with --room")
        args.robot_radius = 0.15 if args.robot_radius is None else args.robot_radius
        args.inflation_radius = 0.5 if args.inflation_radius is None else args.inflation_radius
        args.cost_scaling = 5.0 if args.cost_scaling is None else args.cost_scaling
        if not (0.0 <= args.robot_radius < float("inf") and 0.0 <= args.inflation_radius < float("inf") and 0.0 <= args.cost_scaling < float("inf")):
            ap.error("--robot-radius, --inflation-radius and --cost-scaling are finite numbers >= 0")
        try:
            args.avoid = [parse_avoid(v) for v in args.avoid]
        except ValueError as e:
            ap.error(str(e))
    if args.room is not None:
        if (args.query is not None or args.goal != "object" or args.relation is not None or args.area or args.sound or args.image
                or args.goal_2d or args.view or args.nearest == "path"):
            ap.error("--room goes to a room's centre: no --query, --goal frontier or nbv, --relation, --area, --sound, --image, --goal-2d, --view or "
                     "--nearest path")
        if args.door_width is not None and not (0.0 <= args.door_width < float("inf")):
            ap.error("--door-width is a number of metres >= 0")
        args.room = int(args.room) if args.room.lstrip("+").isdigit() else args.room
        if args.room_names is not None and isinstance(args.room, int):
            ap.error("--room-names belongs to --room NAME")
    elif args.door_width is not None or args.room_names is not None:
        ap.error("--door-width and --room-names belong to --room")
    if args.goal in ("frontier", "nbv"):
        if args.query is not None or args.relation is not None or args.area or args.sound or args.image or args.goal_2d or args.nearest == "path":
            ap.error(f"--goal {args.goal} takes its goal from the explored map: no --query, --relation, --area, --sound, --image, --goal-2d or --nearest path")
        args.known_free = True
    elif args.query is None and args.room is None and args.tour is None:
        ap.error("--query is required (or --goal frontier, --room or --tour)")
    if args.goal == "nbv":
        if args.view or args.view_fraction is not None:
            ap.error("--goal nbv looks for unknown space, not at an object: no --view or --view-fraction")
        args.view_range = 3.0 if args.view_range is None else args.view_range
        args.nbv_count = 1 if args.nbv_count is None else args.nbv_count
        if not (args.view_range > 0.0 and args.view_range < float("inf")) or args.nbv_count < 1:
            ap.error("--view-range is a positive number of metres, --nbv-count is at least 1")
    elif args.nbv_count is not None or args.nbv_conservative:
        ap.error("--nbv-count and --nbv-conservative belong to --goal nbv")
    elif args.view:
        if args.goal == "frontier" or args.relation is not None or args.area or args.sound or args.image or args.goal_2d:
            ap.error("--view looks at the --query object: no --goal frontier, --relation, --area, --sound, --image or --goal-2d")
        args.view_range = 3.0 if args.view_range is None else args.view_range
        args.view_fraction = 0.5 if args.view_fraction is None else args.view_fraction
        if not (args.view_range > 0.0 and args.view_range < float("inf")) or not 0.0 <= args.view_fraction <= 1.0:
            ap.error("--view-range is a positive number of metres, --view-fraction lies in [0, 1]")
    elif args.view_range is not None or args.view_fraction is not None:
        ap.error("--view-range and --view-fraction belong to --view (--view-range also to --goal nbv)")
    if args.render and args.relation == "face":
        ap.error("--relation face plans no path: nothing to --render")
    if args.nearest == "path" and (args.relation is not None or args.area or args.sound or args.image or args.goal_2d):
        ap.error("--nearest path chooses among the --query objects: no --relation, --area, --sound, --image or --goal-2d")
    if args.relation is None and (args.heading is not None or args.query_b is not None):
        ap.error("--heading and --query-b belong to --relation")
    if args.relation is not None:
        if args.area or args.sound or args.image or args.goal_2d:
            ap.error("--relation takes its goal from --query alone: no --area, --sound, --image or --goal-2d")
        if (args.relation == "between") != (args.query_b is not None):
            ap.error("--query-b goes with --relation between, and only with it")
        if args.heading is None:
            ap.error("--relation needs the robot's --heading")
    if not args.customize_obstacles and any(v is not None for v in (args.potential_obstacles, args.obstacles, args.dilate_iter,
                                                                    args.gaussian_sigma)):
        ap.error("--potential-obstacles, --obstacles, --dilate-iter and --gaussian-sigma belong to --customize-obstacles")
    if args.goal_2d and args.image:
        ap.error("--goal-2d takes --query, --area and --sound: an image query has no 2-D map")
    if args.travel and not args.goal_2d:
        ap.error("--travel belongs to --goal-2d")
    if args.travel_from_start and not args.travel:
        ap.error("--travel-from-start belongs to --goal-2d --travel")
    if args.sound_travel and not (args.travel and args.sound):
        ap.error("--sound-travel belongs to --goal-2d --travel with a --sound")
    return args


def parse_avoid(text):
    """--avoid NAME[:RADIUS[:PENALTY]] -> (name, radius in metres, penalty); ValueError with the message for the command line"""
    parts = text.split(":")
    if not 1 <= len(parts) <= 3 or not parts[0].strip():
        raise ValueError(f"--avoid {text!r}: expected NAME[:RADIUS[:PENALTY]]")
    try:
        radius = float(parts[1]) if len(parts) > 1 else 0.3
        penalty = int(parts[2]) if len(parts) > 2 else 200
    except ValueError:
        raise ValueError(f"--avoid {text!r}: RADIUS is a number of metres and PENALTY an integer") from None
    if not (0.0 <= radius < float("inf")) or not 0 <= penalty <= 254:
        raise ValueError(f"--avoid {text!r}: RADIUS is a number of metres >= 0, PENALTY lies in 0 .. 254")
    return parts[0].strip(), radius, penalty


def relation_goal(vm, args, start):
    """the goal point of --relation (left, right, between and the compass four), SystemExit when nothing is in front"""
    if args.relation == "between":
        goal = vm.get_pos_in_between(start, args.heading, args.query, args.query_b)
        missing = goal is None
        what = f"{args.query!r} and {args.query_b!r}"
    else:
        goal = getattr(vm, f"get_{args.relation}_pos")(start, args.heading, args.query)
        missing = goal[0] is None or goal[0] == "stop"
        what = repr(args.query)
    if missing:
        raise SystemExit(f"--relation {args.relation}: no sizeable {what} in front of a robot at {start} heading {args.heading} degrees")
    return [float(goal[0]), float(goal[1])]


def clamp_point(point, rmin, cmin, shape):
    """the full-map point moved into the (H, W) crop that starts at (rmin, cmin)"""
    return [min(max(float(point[0]), float(rmin)), float(rmin) + shape[0] - 1), min(max(float(point[1]), float(cmin)), float(cmin) + shape[1] - 1)]


def obstacle_overrides(args) -> dict:
    """the map_config entries VLMap.customize_obstacle_map reads, for the flags that were given"""
    names = lambda v: [c.strip() for c in v.split(",") if c.strip()]       # noqa: E731
    given = {"potential_obstacle_names": None if args.potential_obstacles is None else names(args.potential_obstacles),
             "obstacle_names": None if args.obstacles is None else names(args.obstacles),
             "dilate_iter": args.dilate_iter, "gaussian_sigma": args.gaussian_sigma}
    return {k: v for k, v in given.items() if v is not None}


def is_cross_modal(args) -> bool:
    return bool(args.area or args.sound or args.image or args.goal_2d or isinstance(getattr(args, "room", None), str))


def room_goal(vm, avlmap, args, start):
    """--room: (the centre of the room, the JSON extras); SystemExit when there is no such room"""
    import numpy as np
    width = 0.9 if args.door_width is None else args.door_width
    if isinstance(args.room, int):
        rooms = vm.get_rooms(width, customized=args.customize_obstacles, known_free=args.known_free)
        if not 1 <= args.room <= rooms.n:
            raise SystemExit(f"--room {args.room}: the map has rooms 1 .. {rooms.n}")
        k = args.room
    else:
        rooms = avlmap.get_rooms(door_width=width, customized=args.customize_obstacles, known_free=args.known_free)
        names = [c.strip() for c in args.room_names.split(",") if c.strip()] if args.room_names else [args.room]
        if args.room not in names:
            names.append(args.room)
        named = avlmap.name_rooms(names, rooms)
        ids = [i + 1 for i, name in enumerate(named) if name == args.room]
        if not ids:
            raise SystemExit(f"--room {args.room!r}: no room gets that name (the rooms' names: {named})")
        scores = avlmap.room_scores[np.array(ids) - 1, names.index(args.room)]
        k = ids[int(np.argmax(scores))]
    here = rooms.room_of(start)
    route = rooms.route(here, k) if here else None
    return rooms.centre(k), {"goal_kind": "room", "room": k, "rooms": rooms.n, "route": route}


def cost_plan(vm, args, obstacles, start, goal):
    """--planner cost: (the path, the JSON extras, the costmap); SystemExit when the start cannot reach the goal"""
    import numpy as np
    from avlmaps_amd import ops
    from avlmaps_amd.utils.navigation_utils import NoPathError
    which = dict(customized=args.customize_obstacles, known_free=args.known_free)
    costmap = vm.get_costmap(args.robot_radius, args.inflation_radius, args.cost_scaling, avoid=args.avoid, **which)
    try:
        walk, price = vm.plan_cost_path(start, goal, costmap=costmap, waypoints=False, with_cost=True, **which)
    except NoPathError as e:
        raise SystemExit(f"--planner cost: {e}") from None
    try:
        clearance = ops.distance_transform_edt(np.asarray(obstacles) != 0)
        least = min(float(clearance[int(p[0]) - int(vm.rmin), int(p[1]) - int(vm.cmin)]) for p in walk) * float(vm.cs)
    except ValueError:                                # a map without obstacles has no clearance
        least = None
    path = [list(p) for p in ops.drop_collinear([tuple(p) for p in walk])]
    return path, {"planner": "cost", "path_cost": price, "min_clearance_m": least}, costmap


def clamp_cell(cell, rmin, cmin, shape):
    """the full-map cell moved into the (H, W) crop that starts at (rmin, cmin)"""
    return [min(max(int(cell[0]), int(rmin)), int(rmin) + int(shape[0]) - 1),
            min(max(int(cell[1]), int(cmin)), int(cmin) + int(shape[1]) - 1)]


def render_plan(vm, obstacles, start, goal, path, view=None, marks=(), costmap=None):
    """(H, W, 3) uint8: the crop of the top-down colour map, obstacle cells (obstacles == 0) at a third of their brightness, the
    cells of `view` (a crop-shaped bool: Viewpoints.mask(), where the object can be seen from, or the cells a next best view would
    see) half-way to cyan, the path in yellow, the start green, the goal red, the full-map cells of `marks` (the later views of a
    tour) orange.  Host drawing on the small image (utils.visualize_utils: integer Bresenham)."""
    import numpy as np
    from avlmaps_amd.utils.visualize_utils import draw_marker, draw_polyline
    r0, c0 = int(vm.rmin), int(vm.cmin)
    H, W = obstacles.shape
    img = np.ascontiguousarray(vm.generate_rgb_topdown_map()[r0:r0 + H, c0:c0 + W])
    blocked = np.asarray(obstacles) == 0
    img[blocked] = img[blocked] // 3
    if costmap is not None:
        price = np.asarray(costmap)
        alpha = (price.astype(np.float32) / 254.0 * 0.6)[..., None]
        red = np.array([255, 0, 0], np.float32)
        tinted = (img.astype(np.float32) * (1.0 - alpha) + red * alpha).astype(np.uint8)
        img = np.where((~blocked & (price > 1))[..., None], tinted, img)
        img[~blocked & (price == 0)] = (96, 0, 0)
    if view is not None:
        seen = np.asarray(view, dtype=bool)
        img[seen] = ((img[seen].astype(np.uint16) + np.array([0, 255, 255], np.uint16)) // 2).astype(np.uint8)
    local = [(float(p[0]) - r0, float(p[1]) - c0) for p in path]
    draw_polyline(img, local, (255, 255, 0))
    for m in marks:
        draw_marker(img, (float(m[0]) - r0, float(m[1]) - c0), (255, 128, 0))
    draw_marker(img, (float(start[0]) - r0, float(start[1]) - c0), (0, 255, 0))
    draw_marker(img, (float(goal[0]) - r0, float(goal[1]) - c0), (255, 0, 0))
    return img


def main(argv=None):
    args = parse_args(argv)

    from avlmaps_amd.apps.common import HashClip, load_config
    from avlmaps_amd.map import VLMap
    from avlmaps_amd.navigator import Navigator
    cfg = load_config(args.config, overrides={f"map_config.{k}": v for k, v in obstacle_overrides(args).items()})
    hashed = args.text_model == "hash"
    avlmap = None
    if is_cross_modal(args):
        from avlmaps_amd.apps.common import HashAudioText
        from avlmaps_amd.map import AVLMap
        avlmap = AVLMap(cfg, data_dir=args.data_dir, area_text_model=HashClip(768) if hashed else None,
                        audio_text_model=HashAudioText() if hashed else None)
        vm, loader = avlmap.vlmap, avlmap
    else:
        vm = loader = VLMap(cfg.map_config, data_dir=args.data_dir)
    if not loader.load_map(args.data_dir):
        if not hashed:
            raise SystemExit(f"no map under {args.data_dir}: run apps.create_map first")
        from avlmaps_amd.apps import create_map
        create_map.main(["--data-dir", args.data_dir, "--features", "hash", "--feat-dim", "64"]
                        + (["--config", args.config] if args.config else []))
        if not loader.load_map(args.data_dir):
            raise SystemExit(1)
    if hashed:
        vm.clip_feat_dim = vm.grid_feat.shape[1]
        vm.clip_model = HashClip(vm.clip_feat_dim)
    elif (args.goal == "object" and args.room is None) or args.customize_obstacles:          # a frontier, view or room goal asks the text tower nothing
        vm._init_clip()
    if args.goal == "object" and args.room is None:
        cats = ([c.strip() for c in args.categories.split(",")] if args.categories
                else (args.tour or [args.query]) + ([args.query_b] if args.query_b else []) + ["other"])
        cats += [a[0] for a in args.avoid if a[0] not in cats]
        vm.init_categories(cats)
    vm.generate_obstacle_map(args.h_min, args.h_max)
    obstacles = vm.get_obstacle_cropped()
    if args.customize_obstacles:
        vm.customize_obstacle_map(cfg.map_config.potential_obstacle_names, cfg.map_config.obstacle_names)
        obstacles = vm.get_customized_obstacle_cropped()
    if args.known_free:
        if vm.first_seen is None:
            raise SystemExit(f"no explored map under {args.data_dir}: run apps.create_map --explored first")
        obstacles = vm.get_known_free_cropped(customized=args.customize_obstacles)
    start = [float(args.start[0]), float(args.start[1])]
    extra = {}
    if args.tour is not None:
        try:
            tour = vm.plan_object_tour(start, args.tour, closed=args.tour_closed, customized=args.customize_obstacles)
        except ValueError as e:
            raise SystemExit(f"--tour: {e}") from None
        out = {"start": start, "tour": tour.names, "skipped": tour.skipped_names, "closed": tour.closed,
               "matrix_length": tour.matrix_length, "driven_length": tour.driven_length,
               "legs": [[[float(r), float(c)] for r, c in leg] for leg in tour.legs]}
        print(json.dumps(out))
        return out
    if args.relation == "face":
        try:
            turn = float(vm.get_delta_angle_to(start, args.heading, args.query))
        except ValueError:
            raise SystemExit(f"--relation face: the map has no {args.query!r} to face") from None
        out = {"query": args.query, "start": start, "relation": "face", "heading": args.heading, "turn_right_deg": turn}
        print(json.dumps(out))
        return out
    if args.relation is not None:
        cell = relation_goal(vm, args, start)
        goal = clamp_point(cell, vm.rmin, vm.cmin, obstacles.shape)
        extra = {"relation": args.relation, "heading": args.heading, "goal_cell": cell}
        if args.query_b:
            extra["query_b"] = args.query_b
    elif args.room is not None:
        goal, extra = room_goal(vm, avlmap, args, start)
    elif args.goal == "frontier":
        frontiers = vm.get_frontiers()
        if len(frontiers[0]) == 0:
            raise SystemExit("--goal frontier: the explored area has no frontier (of at least 5 cells) left")
        goal = None
    elif args.goal == "nbv":
        goal = None
    elif args.view:
        import numpy as np
        viewpoints = vm.get_viewpoints(args.query, max_range=args.view_range, free=np.asarray(obstacles) != 0,
                                       customized=args.customize_obstacles)
        if len(viewpoints.select(args.view_fraction)) == 0:
            raise SystemExit(f"--view: no free cell within {args.view_range} m sees {args.query!r} ({viewpoints.n_targets} voxels tested)")
        goal = None
    elif avlmap is None:
        goal = None if args.nearest == "path" else vm.get_nearest_pos(start, args.query)
    elif args.goal_2d:
        if args.travel:
            query = avlmap.index_goal_2d_sound_travel if args.sound_travel else avlmap.index_goal_2d_travel
            g = query(obj=args.query, area=args.area or None, sound=args.sound or None, want_heat=False,
                      start=start if args.travel_from_start else None)
        else:
            g = avlmap.index_goal_2d(obj=args.query, area=args.area or None, sound=args.sound or None, want_heat=False)
        goal = [int(g.cell[0]), int(g.cell[1])]
        extra = {"goal_value": g.value, "goal_cell": [float(g.cell[0]), float(g.cell[1])]}
    else:
        img = None
        if args.image:
            import numpy as np
            from avlmaps_amd.apps.common import FixedPoseLocalizer
            from avlmaps_amd.utils.mapping_utils import load_rgb_png
            poses = np.loadtxt(vm.pose_path).reshape(-1, 7)
            avlmap.visual_map.localizer = FixedPoseLocalizer(poses[args.image_pose], vm.base2cam_tf)
            img = load_rgb_png(args.image)
        g = avlmap.index_goal(obj=args.query, area=args.area or None, sound=args.sound or None, img=img, want_heat=False)
        goal = clamp_cell(g.cell, vm.rmin, vm.cmin, vm.obstacles_cropped.shape)
        extra = {"goal_voxel": g.voxel, "goal_value": g.value, "goal_cell": [float(g.cell[0]), float(g.cell[1])]}
    nav, costmap = Navigator(), None
    try:
        if args.planner != "cost":
            nav.build_visgraph(obstacles, vm.rmin, vm.cmin)
        if args.planner == "cost":
            path, more, costmap = cost_plan(vm, args, obstacles, start, goal)
            extra = dict(extra, **more)
        elif args.goal == "frontier":
            k, path = nav.plan_to_nearest_frontier(start, frontiers)
            goal = [int(frontiers[0][k, 0]), int(frontiers[0][k, 1])]
            extra = {"goal_kind": "frontier", "frontiers": int(len(frontiers[0])), "frontier_cells": int(frontiers[1][k])}
        elif args.goal == "nbv":
            try:
                tour = vm.plan_exploration(start, args.nbv_count, navigator=nav, max_range=args.view_range,
                                           customized=args.customize_obstacles, opaque_unknown=args.nbv_conservative)
            except ValueError as e:
                raise SystemExit(f"--goal nbv: {e}") from None
            if not tour:
                raise SystemExit(f"--goal nbv: no reachable cell would see any unknown cell within {args.view_range} m: the map is explored")
            goal, path = tour[0][0], tour[0][3]
            extra = {"goal_kind": "nbv", "gain": tour[0][2], "heading_octant": tour[0][1],
                     "views": [{"goal": [float(v[0][0]), float(v[0][1])], "heading_octant": v[1], "gain": v[2]} for v in tour]}
        elif args.view:
            goal, path = vm.get_viewpoint_pos(start, viewpoints, nav if args.nearest == "path" else None, args.view_fraction)
            if args.nearest != "path":
                path = nav.plan_to(start, goal)
            at = int(np.flatnonzero((viewpoints.cells == np.asarray(goal)).all(axis=1))[0])
            extra = {"goal_kind": "viewpoint", "visible": int(viewpoints.visible[at]), "view_targets": viewpoints.n_targets,
                     "view_cells": int(np.count_nonzero(viewpoints.visible))}
        elif args.nearest == "path":
            goal, path = vm.get_nearest_reachable_pos(start, args.query, nav)
        else:
            path = nav.plan_to(start, goal)
    finally:
        nav.close()
    out = {"query": args.query, "start": start, "goal": [float(goal[0]), float(goal[1])],
           "path": [[float(p[0]), float(p[1])] for p in path]}
    out.update(extra)
    if args.render:
        from PIL import Image
        view, marks = viewpoints.mask() if args.view else None, ()
        if args.goal == "nbv":
            import numpy as np
            from avlmaps_amd import ops
            free = np.asarray(vm.get_customized_obstacle_cropped() if args.customize_obstacles else vm.get_obstacle_cropped()) != 0
            eye = np.array([[int(goal[0]) - int(vm.rmin), int(goal[1]) - int(vm.cmin)]], np.int32)
            view = ops.viewshed_seen(free, vm.get_explored_cropped(), eye, int(args.view_range / float(vm.cs)), args.nbv_conservative) != 0
            marks = [v[0] for v in tour[1:]]
        Image.fromarray(render_plan(vm, obstacles, start, goal, path, view, marks, costmap)).save(args.render)
        out["render"] = args.render
    print(json.dumps(out))
    return out


if __name__ == "__main__":
    main()
