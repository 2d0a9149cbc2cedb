"""Precision and recall for distributions (Sajjadi et al. 2018, arXiv:1806.00035), the PRD half of `--eval_metric fvd_prd`
(utils/utils_eval.py:210-219 calls precision_recall_distributions/prd_score.py).  Same functions, signatures, defaults and ValueErrors
as the reference module; host numpy.  `_cluster_into_bins` / `compute_prd_from_embedding` take an optional `seed`, passed to
MiniBatchKMeans as random_state (None: unseeded, as the reference)."""
import numpy as np


def compute_prd(eval_dist, ref_dist, num_angles=1001, epsilon=1e-10):
    """PRD curve of the discrete distribution eval_dist against ref_dist over num_angles equally spaced angles in
    [epsilon, pi/2 - epsilon]: precision(l) = sum_i min(l ref_i, eval_i), recall(l) = precision(l) / l, l = tan(angle); both
    clipped to [0, 1] after a check that neither exceeds 1.001."""
    if not (epsilon > 0 and epsilon < 0.1):
        raise ValueError('epsilon must be in (0, 0.1] but is %s.' % str(epsilon))
    if not (num_angles >= 3 and num_angles <= 1e6):
        raise ValueError('num_angles must be in [3, 1e6] but is %d.' % num_angles)
    slopes = np.tan(np.linspace(epsilon, np.pi / 2 - epsilon, num=num_angles))
    ref = np.asarray(ref_dist)[None, :]
    ev = np.asarray(eval_dist)[None, :]
    precision = np.minimum(ref * slopes[:, None], ev).sum(axis=1)
    recall = precision / slopes
    if max(np.max(precision), np.max(recall)) > 1.001:
        raise ValueError('Detected value > 1.001, this should not happen.')
    return np.clip(precision, 0, 1), np.clip(recall, 0, 1)


def _cluster_into_bins(eval_data, ref_data, num_clusters, seed=None):
    """k-means (MiniBatchKMeans, n_init=10) on the union of both sets; returns the two normalised cluster histograms."""
    from sklearn.cluster import MiniBatchKMeans
    data = np.vstack([eval_data, ref_data])
    labels = MiniBatchKMeans(n_clusters=num_clusters, n_init=10, random_state=seed).fit(data).labels_
    n = len(eval_data)

    def hist(lab):
        return np.histogram(lab, bins=num_clusters, range=[0, num_clusters], density=True)[0]

    return hist(labels[:n]), hist(labels[n:])


def compute_prd_from_embedding(eval_data, ref_data, num_clusters=20, num_angles=1001, num_runs=10, enforce_balance=True, seed=None):
    """PRD of two embedded samples: the mean over num_runs clusterings of compute_prd on the cluster histograms.  With a seed,
    run r uses random_state seed + r."""
    if enforce_balance and len(eval_data) != len(ref_data):
        raise ValueError('The number of points in eval_data %d is not equal to the number of points in ref_data %d. To disable this '
                         'exception, set enforce_balance to False (not recommended).' % (len(eval_data), len(ref_data)))
    eval_data = np.array(eval_data, dtype=np.float64)
    ref_data = np.array(ref_data, dtype=np.float64)
    curves = [compute_prd(*_cluster_into_bins(eval_data, ref_data, num_clusters, None if seed is None else seed + r), num_angles)
              for r in range(num_runs)]
    return np.mean([c[0] for c in curves], axis=0), np.mean([c[1] for c in curves], axis=0)


def _check_pr(precision, recall, beta):
    if not ((precision >= 0).all() and (precision <= 1).all()):
        raise ValueError('All values in precision must be in [0, 1].')
    if not ((recall >= 0).all() and (recall <= 1).all()):
        raise ValueError('All values in recall must be in [0, 1].')
    if beta <= 0:
        raise ValueError('Given parameter beta %s must be positive.' % str(beta))


def _prd_to_f_beta(precision, recall, beta=1, epsilon=1e-10):
    """F_beta = (1 + beta^2) p r / (beta^2 p + r + epsilon) for every pair."""
    _check_pr(precision, recall, beta)
    return (1 + beta**2) * (precision * recall) / ((beta**2 * precision) + recall + epsilon)


def prd_to_max_f_beta_pair(precision, recall, beta=8):
    """(max F_beta, max F_{1/beta}) over the curve: the pair the reference reports as F8 / F1/8."""
    _check_pr(precision, recall, beta)
    return np.max(_prd_to_f_beta(precision, recall, beta)), np.max(_prd_to_f_beta(precision, recall, 1 / beta))
