"""CPU stand-in for rl._engine used by tests/test_host.py to run bench.py's rank launcher and
JSON line without a GPU (RLE_BENCH_STUB=<this file>).  Test infrastructure only."""

import time

import numpy as np

RLE_TD7, RLE_TD3, RLE_SAC = 0, 1, 2


def device_count():
    return 8


def synchronize(device=None):
    pass


def make_config(algo, s, a, h, b, **kw):
    return dict(algo=algo, s=s, a=a, h=h, b=b, **kw)


def init_agent(algo, s, a, h, seed):
    return {"policy": {"l0.weight": np.zeros((2, 3), np.float32), "l0.bias": np.zeros(2, np.float32)}}


def parse_plan(text):
    return dict(item.split("=") for item in filter(None, text.split(",")))


class Replay:
    def __init__(self, n, s, a, lap, device=0):
        self.device = device

    def fill_random(self, n, seed=0):
        pass

    def get_priority(self):
        return np.ones(64, np.float32)


class Engine:
    def __init__(self, cfg, plan=None):
        self.cfg, self.n, self._plan = cfg, 0, dict(plan or {})

    def plan(self):
        return self._plan

    def set_param(self, *a):
        pass

    def bind(self, rep):
        pass

    def graph_stats(self):
        return 23, 13

    def launch_count(self):
        return self.n * 17

    def step_timed(self, n):
        time.sleep(1e-4 * n)
        self.n += n
        return 0.1 * n

    def step_async(self, n):
        time.sleep(1e-4 * n)
        self.n += n

    def synchronize(self):
        pass

    # what --dump-outputs reads back: rows numbered by the step they belong to, None (NaN) in the last column
    def get_info(self, n):
        rows = np.full((n, 8), np.nan, np.float32)
        rows[:, :2] = np.arange(self.n - n + 1, self.n + 1, dtype=np.float32)[:, None]
        return rows

    def last_indices(self):
        return np.arange(self.cfg["b"], dtype=np.int64) + self.n

    def value_bounds(self):
        return np.array([0, 0, -1e8, 1e8], np.float32)

    def get_param(self, net, name, shape=None):
        return np.full(shape, self.n, np.float32)
