from .conformal import TokenConformal, TokenSets  # noqa: F401
from .consistency import (ConsistencyScores, PairCounts, consistency_scores, graph_scores, pairwise_counts,  # noqa: F401
                          pairwise_similarity, word_ids)
from .logits import GenerationScores, generation_scores, token_entropies, transition_scores  # noqa: F401
from .pipeline import compute_uncertainties, compute_uncertainties_batch, eigen_scores  # noqa: F401
from .rauq import (RAUQ, generated_lengths, rauq_batch, rauq_uncertainty, rauq_uncertainty_mean_heads,  # noqa: F401
                   rauq_uncertainty_rollout)
from .scores import eigen_score, semantic_entropy  # noqa: F401

__all__ = ["eigen_score", "semantic_entropy", "rauq_uncertainty", "rauq_uncertainty_mean_heads", "rauq_uncertainty_rollout",
           "RAUQ", "rauq_batch", "generated_lengths", "GenerationScores", "generation_scores", "token_entropies",
           "transition_scores", "compute_uncertainties", "compute_uncertainties_batch", "eigen_scores", "TokenConformal",
           "TokenSets", "PairCounts", "ConsistencyScores", "pairwise_counts", "pairwise_similarity", "graph_scores",
           "consistency_scores", "word_ids"]
