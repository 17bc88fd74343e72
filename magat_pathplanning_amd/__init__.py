"""MI355X-native MAGAT batched graph-attention forward (drop-in for the reference's
DecentralPlannerGATNet / GraphFilterBatchAttentional).  See DESIGN.md and INTEGRATION.md."""
from .graphml import (GraphFilterBatch, GraphFilterBatchAttentional, GraphFilterBatchAttentional_Origin,  # noqa: F401
                      GraphFilterBatchSimilarityAttentional)
from .planner import DecentralPlannerBottleneckNet, DecentralPlannerGATNet, DecentralPlannerNet  # noqa: F401
from .expert import expert_radius, expert_samples, expert_schedule, expert_stats, flatten_samples, pack_schedules  # noqa: F401
from .cases import generate_cases, valid_cases  # noqa: F401
from .mapf import adopt_bounded, audit_schedules, cbs_cases, ecbs_cases, ecbs_cases_wide, certified, certified_pack, improve_schedules, pack_cases, plan_prioritized, solve_cases, solved_pack  # noqa: F401
from .simulator import (GUIDANCE_MODES, BatchedEpisode, GraphEdges, batched_edges, batched_fov_states, batched_gso,  # noqa: F401
                        new_agent_view, replayed_semi_states)
from .memory import ExpertMemory, online_expert  # noqa: F401
from .loss import ActionLoss, head_loss  # noqa: F401
from .rollout import EpisodePool, evaluate_cases, reference_maxstep, summarize_rollouts  # noqa: F401

__all__ = ["DecentralPlannerGATNet", "DecentralPlannerNet", "DecentralPlannerBottleneckNet", "GraphFilterBatchAttentional", "GraphFilterBatchAttentional_Origin", "GraphFilterBatchSimilarityAttentional", "GraphFilterBatch",
           "BatchedEpisode", "batched_fov_states", "batched_gso", "batched_edges", "GraphEdges", "new_agent_view", "replayed_semi_states", "GUIDANCE_MODES",
           "pack_schedules", "expert_schedule", "expert_radius", "expert_stats", "expert_samples", "flatten_samples",
           "plan_prioritized", "solve_cases", "solved_pack", "pack_cases", "improve_schedules", "audit_schedules", "certified", "certified_pack", "cbs_cases", "ecbs_cases", "ecbs_cases_wide", "adopt_bounded",
           "generate_cases", "valid_cases", "ExpertMemory", "online_expert",
           "EpisodePool", "evaluate_cases", "reference_maxstep", "summarize_rollouts", "ActionLoss", "head_loss"]
