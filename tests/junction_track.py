"""The junction track of the env tests (tests/test_env_gpu.py, test_rollout_f64_gpu.py) and of the table compiler's host test
(tests/test_track_tables_host.py): needs nothing but json."""


def _junction_track_json(path):
    """A box (outer loop) and an inner polyline T0 -> T1 -> A -> B -> C -> D whose first point lies in the INTERIOR of the box's
    bottom wall (a T-junction: two walls touch without being chain neighbours) and whose segments AB and CD CROSS each other (an
    X): both are outside what a float32 selector can order by looking at chain neighbours."""
    import json
    W, H = 1280.0, 720.0
    n = lambda pts: [[x / W, y / H] for x, y in pts]
    outer = [(50, 50), (650, 50), (650, 350), (50, 350), (50, 50)]
    inner = [(300, 50), (300, 150), (420, 180), (520, 280), (520, 180), (420, 280)]
    gates = [(60, 60), (61, 60), (70, 60), (71, 60)]
    json.dump({"outer_track_points": n(outer), "inner_track_points": n(inner), "reward_gates": n(gates),
               "initial_position": [150 / W, 200 / H], "initial_angle": 0.0}, open(path, "w"))
    return path
