"""marllb_amd — MI355X-native vectorised load-balancing RL environment (lbsim).

The hot path of the MARLLB reference (problem-03 LoadBalanceEnv.step/reset + problem-01 reservoir
feature collector) as hand-written gfx950 HIP kernels behind a C ABI (include/lbsim.h,
liblbsim.so), with the reference's Gym-style API on top.
"""
from .env import (FEATURE_NAMES, GROUND_TRUTH_COLUMNS, POOL_PS_STATE_COLUMNS, PS_STATE_COLUMNS,
                  DeviceSnapshot, LoadBalanceEnv, LoadBalanceEnvGym, VecLoadBalanceEnv,
                  make_config)
from .multi_agent import MultiAgentLoadBalanceEnv, VecMultiAgentLoadBalanceEnv
from .pools import VecServerPoolEnv
from .randomize import (burst_schedule, diurnal_schedule, outage_schedule,
                        rolling_restart_schedule, sample_ack_interval, sample_action_delay,
                        sample_cluster_sizes,
                        sample_cross_traffic, sample_pool_arrival_rates, sample_rates,
                        sample_server_workers, schedule_phase)
from .spaces import Box, MultiDiscrete
from .workload import (TABLE_BINS, bounded_pareto_table, constant_table, empirical_table,
                       exponential_table, hyperexp_table, lognormal_table, quantile_table,
                       sample_table_ids, table_bin, table_cv2, table_mean, weibull_table)

__all__ = ["FEATURE_NAMES", "LoadBalanceEnv", "LoadBalanceEnvGym", "VecLoadBalanceEnv",
           "MultiAgentLoadBalanceEnv", "VecMultiAgentLoadBalanceEnv", "make_config", "Box",
           "MultiDiscrete", "sample_rates", "schedule_phase", "diurnal_schedule",
           "burst_schedule", "DeviceSnapshot", "TABLE_BINS", "table_bin", "quantile_table",
           "exponential_table", "bounded_pareto_table", "lognormal_table", "hyperexp_table",
           "weibull_table", "constant_table", "empirical_table", "table_mean", "table_cv2",
           "sample_table_ids", "sample_cluster_sizes", "outage_schedule",
           "rolling_restart_schedule", "sample_cross_traffic", "sample_server_workers",
           "sample_action_delay", "GROUND_TRUTH_COLUMNS", "PS_STATE_COLUMNS", "VecServerPoolEnv",
           "sample_pool_arrival_rates", "POOL_PS_STATE_COLUMNS", "sample_ack_interval"]
__version__ = "0.1.0"
