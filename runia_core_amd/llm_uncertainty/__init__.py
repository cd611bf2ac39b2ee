from .logits import GenerationScores, generation_scores, token_entropies, transition_scores  # noqa: F401
from .rauq import RAUQ, rauq_uncertainty, rauq_uncertainty_mean_heads, rauq_uncertainty_rollout  # noqa: F401
from .scores import eigen_score, semantic_entropy  # noqa: F401

__all__ = ["eigen_score", "semantic_entropy", "rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout",
           "RAUQ", "GenerationScores", "generation_scores", "token_entropies", "transition_scores"]
