"""Data selection by predictive scores and by k-means clusters (the reference's
psvi/inference/utils.py: 221-552, 616-1265, 1381-1607) on the HIP library:

  MeanFieldVI      utils.py:221-452    MFVI pretraining on the training set, with forgetting events
  WeightedSubset   utils.py:616-626    a Subset whose items carry (idx, data, target, weight)
  Selection        utils.py:629-729    get_subset / get_weighted_subset / pretrain
  RandomSelection  utils.py:749-786    a random subset per class
  ScoreSelection   utils.py:941-1084   the top rows per class by a predictive score
  ScoreCalculator  utils.py:1088-1113  the three scores of a probability matrix (torch)
  CoresetSelect    utils.py:1419-1607  picks the selection method and runs it
  KmeansCluster    utils.py:455-552    k-means per class (or over all rows), points per cluster
  KmeansSelection  utils.py:789-938    rows picked at random inside k-means clusters
  KmeansScoreSelection      utils.py:1116-1265  rows picked inside clusters by their scores
  WeightedKmeansSelection   utils.py:1381-1416  k-means rows weighted by their entropy score

The training half is ``_MFVIStepper`` (psvi_elbo_grad + torch-Adam); every
predictive pass is ONE psvi_predict_scores launch (psvi.runtime.predict_scores):
``MeanFieldVI.after_epoch`` over the training set with the forgetting state,
``MeanFieldVI.test`` per shuffled test batch with the statistics, and
``ScoreSelection._get_uncertainty_score`` over the training set with
``rows_per_draw = 128``.  The per-class ``torch.topk`` and the "remainder on the
last class" split stay in torch.  There is no CPU fallback.
Reference behaviours kept:

* ``Selection.pretrain`` passes ``forgetting_flag=``, which ``MeanFieldVI``
  swallows in ``**kwargs`` (its parameter is ``forgetting_score_flag``): through
  ``CoresetSelect`` the ``"forgetting"`` scores are all zero and top-k picks
  whatever torch.topk returns for a constant vector.  ``MeanFieldVI(forgetting_score_flag=True)`` called directly
  counts the events.
* ``train_an_epoch`` walks an unshuffled loader with scale ``n_train / B`` (the
  last batch its own B); ``test`` a shuffled one; a test at ``i % log_every ==
  0`` and after the last iteration.
* ``after_epoch`` updates ``forgetting += last_acc > correct``, ``last_acc =
  correct``, ``never_learnt = min(never_learnt, 1 - correct)`` with fresh weights
  per minibatch; at the end ``forgetting = max(total_iterations * never_learnt,
  forgetting)``.
* ``get_weighted_subset`` permutes the chosen indices with
  ``np.random.permutation`` and weights them ``n_train / n_coreset``.
* ``select`` saves the scores it computed to
  ``{score_type}_{dnm}_10_{seed}.csv`` and takes ``num_pseudo // nc`` rows per
  class, the remainder on the last class.
Divergences (DESIGN §4 "MFVI selection", §9): ``loaded=True`` reads
``score_psvi_{dnm}_{seed}.csv`` with numpy by column name when the file exists
and computes the scores otherwise; ``"el2n"`` is ``_el2n_score`` of the one
pretrained net (the reference averages ten per-seed files nothing writes); a
``data_folder`` / ``data_path`` of None skips the score and checkpoint files;
kmeans_gradient, submodular (faiss / the submodular package),
architecture="lenet" and log_pseudodata raise NotImplementedError.
``scored_random_*`` falls out of ScoreSelection (RandomScoreSelection) and is
ported.
K-means (DESIGN §4 "K-means selection"): the reference clusters with sklearn on
the CPU; here every clustering is one ``psvi.runtime.kmeans`` call
(psvi_kmeans: Philox k-means++ with one candidate per centre, fp64 Lloyd,
empty clusters kept), so the clusters are a k-means solution, not sklearn's.
That is why ``CoresetSelect(clustering=None)`` still refuses kmeans,
scored_kmeans_* and weighted_kmeans as before, and ``clustering="hip"`` opens
them.  Raw rows only (``embedding_flag=False``): the LeNet embeddings stay
refused with the architecture.  ``loaded=True`` reads
``embedding_{dnm}_{seed}.csv`` with numpy when the file exists and uses the
dataset's rows otherwise.  ``_set_num_clusters`` raises ValueError where the
reference returns None (``multiple_pts`` with a num_pseudo outside {30, 50,
80, 100}).  The reference's WeightedKmeansSelection cannot run (it calls
``get_arbitrary_pts()`` without its argument and builds the subset from
``self.p``): ported with ``total_pts=self.num_pseudo`` and
``indices=self.core_idc``; its weights are normalised to sum to n_train like
every other selection's (the reference's factor makes them sum to n_train /
n_coreset).  The picks inside clusters stay on numpy's global
generator, as in the reference.
Optional hook: ``eps_source(n)`` supplies every draw of n floats (a training
step's or one predictive minibatch's noise, in the reference's order).
"""
import os
import random
import re
import time
from typing import List

import numpy as np
import torch
import torch.nn.functional as F
from torch.utils.data import DataLoader, Subset

from ..models import categorical_fn

__all__ = ["MeanFieldVI", "WeightedSubset", "Selection", "RandomSelection", "ScoreSelection",
           "RandomScoreSelection", "ScoreCalculator", "CoresetSelect", "KmeansCluster",
           "KmeansSelection", "KmeansScoreSelection", "WeightedKmeansSelection",
           "sample_multinomial"]

_NO_KMEANS = ("kmeans", "kmeans_gradient", "submodular", "weighted_kmeans",
              "scored_kmeans_el2n", "scored_kmeans_forgetting", "scored_kmeans_entropy",
              "scored_kmeans_least_confidence")
# what clustering="hip" opens: the methods whose only missing piece was k-means
_HIP_KMEANS = tuple(m for m in _NO_KMEANS if m not in ("kmeans_gradient", "submodular"))


def _B():
    from . import baselines
    return baselines


def _rows(dataset):
    """(x, y) of a whole dataset in index order, as tensors."""
    if hasattr(dataset, "data") and hasattr(dataset, "targets"):
        return torch.as_tensor(dataset.data), torch.as_tensor(dataset.targets)
    if hasattr(dataset, "tensors"):
        return dataset.tensors[0], dataset.tensors[1]
    items = [dataset[i] for i in range(len(dataset))]
    return (torch.stack([torch.as_tensor(a[0]) for a in items]),
            torch.as_tensor([float(a[1]) for a in items]))


def _refuse_net(architecture, log_pseudodata=False):
    if architecture == "lenet":
        raise NotImplementedError('architecture="lenet": psvi_predict_scores runs the affine '
                                  "mean-field stacks only")
    if log_pseudodata:
        raise NotImplementedError("log_pseudodata (grid predictions) is not on the HIP path")


class MeanFieldVI:
    """run_mfvi as a class (utils.py:221-452), with the forgetting events of
    the training rows."""

    def __init__(self, xt=None, yt=None, mc_samples=4, data_minibatch=128, num_epochs=100,
                 log_every=10, N=None, D=None, lr0net=1e-3, mul_fact=2, seed=0,
                 distr_fn=categorical_fn, architecture=None, n_hidden=None, nc=2,
                 log_pseudodata=False, train_dataset=None, test_dataset=None, init_sd=None,
                 forgetting_score_flag=False, data_path=None, load_from_saved=False, dnm=None,
                 eps_source=None, **kwargs):
        _refuse_net(architecture, log_pseudodata)
        self.mc_samples, self.data_minibatch = mc_samples, data_minibatch
        self.num_epochs, self.log_every = num_epochs, log_every
        self.N, self.D, self.lr0net, self.seed = N, D, lr0net, seed
        self.distr_fn, self.architecture, self.n_hidden, self.nc = distr_fn, architecture, n_hidden, nc
        self.log_pseudodata = log_pseudodata
        self.train_dataset, self.test_dataset = train_dataset, test_dataset
        self.init_sd, self.mul_fact = init_sd, mul_fact
        self.forgetting_score_flag = forgetting_score_flag
        self.data_path, self.load_from_saved, self.dnm = data_path, load_from_saved, dnm
        self.eps_source = eps_source

    def before_train(self):
        B = _B()
        self.device = B._device()
        random.seed(self.seed), np.random.seed(self.seed), torch.manual_seed(self.seed)
        self.net = B.set_up_model(architecture=self.architecture, D=self.D, n_hidden=self.n_hidden,
                                  nc=self.nc, mc_samples=self.mc_samples,
                                  init_sd=self.init_sd).to(self.device)
        # the unshuffled train loader: the rows in index order, on the device
        x, y = _rows(self.train_dataset)
        self.n_train = int(x.shape[0])
        self.x_train = x.to(self.device, torch.float32).reshape(self.n_train, -1).contiguous()
        self.y_train = y.to(self.device)
        self.test_loader = DataLoader(self.test_dataset, batch_size=self.data_minibatch,
                                      pin_memory=True, shuffle=True)
        self.stepper = B._MFVIStepper(self.net, self.device, self.lr0net, self.seed,
                                      self.eps_source)
        self.total_iterations = self.mul_fact * self.num_epochs
        self.nlls_mfvi, self.accs_mfvi, self.times_mfvi, self.elbos_mfvi = [], [], [0], []
        self.t_start = time.time()
        self.forgetting_events = torch.zeros(self.n_train, device=self.device)
        self.last_acc = torch.zeros(self.n_train, device=self.device)
        self.never_learnt_events = torch.ones(self.n_train, device=self.device)

    def train_an_epoch(self):
        """One _MFVIStepper.step per minibatch of the unshuffled loader."""
        losses = []
        for lo in range(0, self.n_train, self.data_minibatch):
            xb = self.x_train[lo:lo + self.data_minibatch]
            yb = self.y_train[lo:lo + self.data_minibatch]
            losses.append(self.stepper.step(xb, yb, self.n_train / xb.shape[0]))
        self.elbos_mfvi.extend((-torch.cat([l.reshape(1) for l in losses])).tolist())

    def test(self):
        """One psvi_predict_scores launch per batch of the shuffled test loader."""
        total, stats = 0, torch.zeros(2, dtype=torch.float64, device=self.device)
        for xt, yt in self.test_loader:
            stats += self.stepper.predict(xt, yt, int(xt.shape[0]), stats=True)["stats"]
            total += yt.size(0)
        corrects, test_nll = stats.tolist()
        self.times_mfvi.append(self.times_mfvi[-1] + time.time() - self.t_start)
        self.nlls_mfvi.append(test_nll / float(total))
        self.accs_mfvi.append(corrects / float(total))

    def after_epoch(self):
        """The forgetting events (utils.py:359-387): one launch over the training
        set, fresh weights per minibatch, the three state vectors updated in it."""
        if not self.forgetting_score_flag:
            return
        self.stepper.predict(self.x_train, self.y_train, self.data_minibatch,
                             state=(self.last_acc, self.forgetting_events,
                                    self.never_learnt_events))

    def run(self):
        self.before_train()
        if self.load_from_saved and self.load():
            return
        for i in range(self.total_iterations):
            self.train_an_epoch()
            self.after_epoch()
            if i % self.log_every == 0 or i == self.total_iterations - 1:
                self.test()
        if self.forgetting_score_flag:
            self.forgetting_events = torch.max(self.total_iterations * self.never_learnt_events,
                                               self.forgetting_events)
        self.stepper.sync_model()
        self.save()

    def _get_net_fname(self):
        return os.path.join(self.data_path, f"net_state_dict_{self.dnm}_{self.architecture}_"
                                            f"{self.num_epochs}_{self.seed}.pt")

    def _get_forgetting_fname(self):
        return os.path.join(self.data_path, f"forgetting_{self.dnm}_{self.architecture}_"
                                            f"{self.num_epochs}_{self.seed}.pt")

    def save(self):
        if self.data_path is None:
            return
        torch.save(self.net.state_dict(), self._get_net_fname())
        torch.save(self.forgetting_events, self._get_forgetting_fname())

    def load(self):
        if self.data_path is None:
            return False
        net_fname, forgetting_fname = self._get_net_fname(), self._get_forgetting_fname()
        if not (os.path.exists(net_fname) and os.path.exists(forgetting_fname)):
            return False
        self.forgetting_events = torch.load(forgetting_fname, map_location=self.device)
        self.net.load_state_dict(torch.load(net_fname, map_location=self.device))
        self.stepper = _B()._MFVIStepper(self.net, self.device, self.lr0net, self.seed,
                                         self.eps_source)
        return True


class WeightedSubset(Subset):
    def __init__(self, dataset, indices, weights) -> None:
        self.dataset = dataset
        assert len(indices) == len(weights)
        self.indices = indices
        self.weights = weights

    def __getitem__(self, idx):
        data, target = self.dataset[self.indices[idx]]
        return idx, data, target, self.weights[idx]

    def __getitems__(self, indices):
        # a DataLoader batches a Subset through this: keep the four-field items
        return [self[i] for i in indices]


class Selection:
    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False):
        self.train_dataset = train_dataset
        self.num_pseudo = num_pseudo
        self.nc = nc
        self.seed = seed
        self.forgetting_flag = forgetting_flag
        self.core_idc = []
        self.wt_vec = None
        self.chosen_dataset = None
        self.eps_source = None

    def select(self) -> List[int]:
        raise NotImplementedError("Child class must implement selection")

    def get_subset(self):
        self.core_idc = self.select()
        self.chosen_dataset = Subset(self.train_dataset, self.core_idc)
        return self.chosen_dataset

    def get_weighted_subset(self, wt_vec=None):
        if len(self.core_idc) == 0:
            self.core_idc = self.select()
            self.core_idc = list(np.random.permutation(self.core_idc))
        if self.wt_vec is None:
            n_coreset = len(self.core_idc)
            self.wt_vec = len(self.train_dataset) / n_coreset * torch.ones(n_coreset)
        self.chosen_dataset = WeightedSubset(dataset=self.train_dataset, indices=self.core_idc,
                                             weights=self.wt_vec)
        return self.chosen_dataset

    def pretrain(self, test_dataset, architecture, D, n_hidden, distr_fn, mc_samples, init_sd,
                 data_minibatch, pretrain_epochs, lr0net, log_every, data_folder,
                 load_from_saved, dnm):
        """MFVI on the training set; ``forgetting_flag=`` is not a parameter of
        MeanFieldVI (module docstring)."""
        self.pretrained_vi = MeanFieldVI(
            mc_samples=mc_samples, data_minibatch=data_minibatch, num_epochs=pretrain_epochs,
            log_every=log_every, N=len(self.train_dataset), D=D, lr0net=lr0net, mul_fact=2,
            seed=self.seed, distr_fn=categorical_fn, architecture=architecture,
            n_hidden=n_hidden, nc=self.nc, train_dataset=self.train_dataset,
            test_dataset=test_dataset, init_sd=init_sd, forgetting_flag=self.forgetting_flag,
            data_path=data_folder, load_from_saved=load_from_saved, dnm=dnm,
            eps_source=self.eps_source)
        self.pretrained_vi.run()
        self.pretrained_net = self.pretrained_vi.net

    def _class_split(self, num_pts):
        """(class, its row indices, how many to take): num_pts // nc per class,
        the remainder on the last one."""
        n_train = len(self.train_dataset)
        targets = np.asarray(torch.as_tensor(self.train_dataset.targets))
        per_class = num_pts // self.nc
        for c in range(self.nc):
            idx_c = np.arange(n_train)[targets == c]
            yield c, idx_c, (num_pts - (self.nc - 1) * per_class if c == self.nc - 1 else per_class)


class RandomSelection(Selection):
    def __init__(self, train_dataset, num_pseudo, nc, seed):
        super().__init__(train_dataset, num_pseudo, nc, seed)

    def select(self):
        core_idc = []
        for _, idx_c, num_pts in self._class_split(self.num_pseudo):
            core_idc = core_idc + np.random.choice(idx_c, num_pts, replace=False).tolist()
        return core_idc

    def pretrain(self, *args, **kwargs):
        pass


class ScoreSelection(Selection):
    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False,
                 score_type="least_confidence", data_folder=None, dnm="MNIST", loaded=False,
                 eps_source=None):
        self.data_folder = data_folder
        self.dnm = dnm
        if score_type == "forgetting":
            forgetting_flag = True
        super().__init__(train_dataset, num_pseudo, nc, seed, forgetting_flag)
        allowed_scores = ["least_confidence", "entropy", "el2n", "forgetting"]
        if score_type not in allowed_scores:
            raise ValueError(f"{score_type} not in {allowed_scores}")
        self.score_type = score_type
        self.loaded = loaded
        self.eps_source = eps_source

    def _scores(self):
        """loaded: the saved PSVI scores when their file exists, else computed."""
        score_arr = self._get_uncertainty_score_loaded() if self.loaded else None
        if score_arr is None:
            score_arr = self._get_uncertainty_score()
            self._save_uncertainty_score(score_arr)
        return score_arr

    def _top_per_class(self, score_arr, num_pts):
        core_idc = []
        for _, idx_c, k in self._class_split(num_pts):
            top_k = torch.topk(score_arr[idx_c], k).indices
            core_idc = core_idc + idx_c[top_k.detach().numpy().tolist()].tolist()
        return core_idc

    def select(self):
        return self._top_per_class(self._scores(), self.num_pseudo)

    def _get_uncertainty_score(self):
        """One launch over the training set, 128 rows per draw (utils.py:992-1023;
        "el2n" in the _el2n_score form on the pretrained net)."""
        if self.score_type == "forgetting":
            return self.pretrained_vi.forgetting_events.detach().cpu()
        B = _B()
        vi = getattr(self, "pretrained_vi", None)
        stepper = B._MFVIStepper(self.pretrained_net, B._device(), 0.0, self.seed, self.eps_source)
        if vi is not None and hasattr(vi, "stepper"):
            stepper.offset = vi.stepper.offset  # the Philox stream goes on
        key = {"least_confidence": "least_conf", "entropy": "entropy", "el2n": "el2n"}[
            self.score_type]
        x, y = _rows(self.train_dataset)
        score = stepper.predict(x, y, 128, want=(key,))[key]
        if vi is not None and hasattr(vi, "stepper"):
            vi.stepper.offset = stepper.offset
        return score.cpu()

    def _get_uncertainty_score_loaded(self):
        if self.data_folder is None:
            return None
        fname = os.path.join(self.data_folder, f"score_psvi_{self.dnm}_{self.seed}.csv")
        if not os.path.exists(fname):
            return None
        table = np.genfromtxt(fname, delimiter=",", names=True)
        return torch.from_numpy(np.atleast_1d(table[self.score_type]).astype(np.float64))

    def _get_score_fname(self, seed=None):
        seed = self.seed if seed is None else seed
        return os.path.join(self.data_folder, f"{self.score_type}_{self.dnm}_10_{seed}.csv")

    def _save_uncertainty_score(self, score_arr):
        if self.data_folder is not None:
            np.savetxt(self._get_score_fname(), score_arr.numpy())

    def _least_confidence_score(self, outputs_prob):
        return ScoreCalculator(outputs_prob, None, self.nc).least_confidence_score()

    def _entropy_score(self, outputs_prob):
        return ScoreCalculator(outputs_prob, None, self.nc).entropy_score()

    def _el2n_score(self, outputs_prob, target):
        return ScoreCalculator(outputs_prob, target, self.nc).el2n_score()


class RandomScoreSelection(ScoreSelection):
    """Half the rows at random, half by score (utils.py:1268-1330)."""

    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False,
                 score_type="least_confidence"):
        super().__init__(train_dataset, num_pseudo, nc, seed, forgetting_flag, score_type)

    def select(self):
        random_core_idc = self._make_random_selection()
        return random_core_idc + self._make_scored_selection(self.num_pseudo - len(random_core_idc))

    def _make_random_selection(self):
        per_class = max(self.num_pseudo // (2 * self.nc), 1)
        last = max(self.num_pseudo // 2 - (self.nc - 1) * per_class, 1)
        core_idc = []
        for c, idx_c, _ in self._class_split(self.num_pseudo):
            k = last if c == self.nc - 1 else per_class
            core_idc = core_idc + np.random.choice(idx_c, k, replace=False).tolist()
        return core_idc

    def _make_scored_selection(self, num_scored_pts):
        return self._top_per_class(self._get_uncertainty_score(), num_scored_pts)


class KmeansCluster:
    """K-means of the rows, per class (balanced) or over all of them
    (utils.py:455-552), each clustering one psvi.runtime.kmeans call: max_iter
    300 and tol = 1e-4 mean_f var_i(x_if) (sklearn's defaults and its tol
    rule), the Philox stream (seed, 0) advanced by the words each call used."""

    def __init__(self, x, y, num_classes=2, balance=True, seed=None, dist="euclidean"):
        valid_dist = ["cosine", "euclidean"]
        if dist not in valid_dist:
            raise ValueError(f"{dist} is not one ov valid dist: {valid_dist}")
        self.x, self.y = x, y
        self.balance, self.num_classes, self.dist = balance, num_classes, dist
        self.kmeans_dict = []
        self.cluster_centers = []
        self.seed = int(time.time()) if seed is None else seed

    def set_num_clusters(self, num_clusters):
        self.num_clusters = num_clusters
        self.pts_per_class = max(int(np.floor(num_clusters / self.num_classes)), 2)

    def run_kmeans(self):
        if self.balance:
            self.run_kmeans_balanced()
        else:
            self.run_kmeans_unbalanced()

    def _rows(self):
        """The rows as (n, D) float32 (3-d data flattened), unit L2 rows under
        the cosine distance (a zero row stays zero), on the HIP device."""
        x = torch.as_tensor(self.x)
        x = x.reshape(x.shape[0], -1).to(torch.float32)
        if torch.cuda.is_available():
            x = x.to("cuda")
        if self.dist == "cosine":
            norm = torch.linalg.vector_norm(x, dim=1, keepdim=True)
            x = x / torch.where(norm > 0, norm, torch.ones_like(norm))
        return x.contiguous()

    def _cluster(self, rows, indices, K):
        from .. import runtime

        tol = 1e-4 * float(rows.double().var(dim=0, unbiased=False).mean())
        out = runtime.kmeans(rows, K, seed=self.seed, offset=self._offset, max_iter=300, tol=tol)
        self._offset += out["consumed"]
        this_kmeans_dict = {}
        for counter, label in enumerate(torch.as_tensor(out["labels"]).cpu().tolist()):
            this_kmeans_dict.setdefault(label, []).append(int(indices[counter]))
        self.kmeans_dict.append(this_kmeans_dict)
        self.cluster_centers.append(torch.as_tensor(out["centres"]).cpu().numpy())

    def run_kmeans_balanced(self):
        self.kmeans_dict, self.cluster_centers, self._offset = [], [], 0
        x, y = self._rows(), np.asarray(torch.as_tensor(self.y).int())
        for class_index in range(self.num_classes):
            indices = np.where(y == class_index)[0]
            sel = torch.as_tensor(indices, device=x.device)
            self._cluster(x[sel].contiguous(), indices, self.pts_per_class)

    def run_kmeans_unbalanced(self):
        self.kmeans_dict, self.cluster_centers, self._offset = [], [], 0
        x = self._rows()
        self._cluster(x, np.arange(x.shape[0]), self.num_clusters)

    def get_arbitrary_pts(self, total_pts):
        """total_pts // num_clusters rows from every non-empty cluster, the
        remainder on the last, by np.random.choice."""
        pts_per_cluster = [total_pts // self.num_clusters] * self.num_clusters
        pts_per_cluster[-1] = total_pts - sum(pts_per_cluster[:-1])
        core_idcs, counter = [], 0
        for this_kmeans_dict in self.kmeans_dict:
            for k in this_kmeans_dict.keys():
                if len(this_kmeans_dict[k]) > 0:
                    num_pts = pts_per_cluster[counter]
                    counter += 1
                    core_idcs = core_idcs + list(
                        np.random.choice(this_kmeans_dict[k], num_pts, replace=False))
        return [int(i) for i in core_idcs]


def sample_multinomial(pval, k):
    """The k entries drawn most often among 2 N multinomial draws (utils.py:732-744)."""
    pval = np.array(pval) if isinstance(pval, list) else pval
    N = pval.shape[0]
    try:
        samples = np.random.multinomial(2 * N, pval, size=1)[0]
        return np.argsort(samples)[-k:]
    except Exception:
        return np.random.choice(a=N, size=k, replace=False)


def _kmeans_num_clusters(sel):
    if not sel.multiple_pts:
        return sel.num_pseudo
    table = {30: 30, 50: 50, 80: 20, 100: 20}
    if sel.num_pseudo not in table:
        raise ValueError(f"multiple_pts=True has cluster counts for num_pseudo in {sorted(table)} "
                         f"only (got {sel.num_pseudo}): the reference returns None there")
    return table[sel.num_pseudo]


def _kmeans_rows(sel):
    """The rows to cluster: embedding_{dnm}_{seed}.csv when ``loaded`` and the
    file exists, else the dataset's own rows."""
    if sel.embedding_flag:
        raise NotImplementedError("embedding_flag=True (the LeNet embeddings) is not on the HIP path")
    if sel.loaded and sel.data_folder is not None:
        fname = os.path.join(sel.data_folder, f"embedding_{sel.dnm}_{sel.seed}.csv")
        if os.path.exists(fname):
            return torch.from_numpy(np.atleast_2d(np.loadtxt(fname, delimiter=",")))
    return _rows(sel.train_dataset)[0]


def _run_kmeans(sel):
    cluster = KmeansCluster(x=_kmeans_rows(sel), y=torch.as_tensor(sel.train_dataset.targets),
                            num_classes=sel.nc, seed=sel.seed, dist=sel.dist)
    cluster.set_num_clusters(sel._set_num_clusters())
    cluster.run_kmeans()
    return cluster


class KmeansSelection(Selection):
    """num_pseudo rows picked at random inside the k-means clusters of every
    class (utils.py:789-938).  No pretraining: the raw rows are clustered."""

    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False,
                 embedding_flag=False, dist="euclidean", data_folder=None, dnm="MNIST",
                 multiple_pts=True, loaded=True):
        super().__init__(train_dataset, num_pseudo, nc, seed, forgetting_flag)
        self.embedding_flag, self.dist = embedding_flag, dist
        self.data_folder, self.dnm = data_folder, dnm
        self.multiple_pts, self.loaded = multiple_pts, loaded

    def select(self):
        self.kmeans_cluster = _run_kmeans(self)
        return self.kmeans_cluster.get_arbitrary_pts(self.num_pseudo)

    def _set_num_clusters(self):
        return _kmeans_num_clusters(self)

    def pretrain(self, *args, **kwargs):
        pass


class KmeansScoreSelection(ScoreSelection):
    """int(num_pseudo / clusters) rows per k-means cluster, drawn by their
    predictive scores (utils.py:1116-1265): in proportion to score + alpha
    (choose_difficult) or to 1 / (score + alpha + 1e-20)."""

    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False,
                 score_type="least_confidence", embedding_flag=False, dist="euclidean",
                 data_folder=None, dnm="MNIST", multiple_pts=True, alpha=0, loaded=False,
                 choose_difficult=True):
        super().__init__(train_dataset, num_pseudo, nc, seed, forgetting_flag, score_type,
                         data_folder, dnm, loaded)
        self.embedding_flag, self.dist, self.alpha = embedding_flag, dist, alpha
        self.multiple_pts, self.choose_difficult = multiple_pts, choose_difficult

    def select(self):
        self.score_arr = self._scores()
        self.kmeans_cluster = _run_kmeans(self)
        return self._combine_kmeans_score()

    def _set_num_clusters(self):
        return _kmeans_num_clusters(self)

    def _combine_kmeans_score(self):
        pts_per_cluster = int(self.num_pseudo / self._set_num_clusters())
        score = np.asarray(self.score_arr, dtype=np.float64)
        core_idcs = []
        for this_kmeans_dict in self.kmeans_cluster.kmeans_dict:
            for k in this_kmeans_dict.keys():
                indices = this_kmeans_dict[k]
                if len(indices) > 0:
                    sub = score[indices] + self.alpha
                    if not self.choose_difficult:
                        sub = 1.0 / (sub + 1e-20)
                    chosen = sample_multinomial(pval=sub / sub.sum(), k=pts_per_cluster)
                    core_idcs = core_idcs + [indices[int(j)] for j in chosen]
        return core_idcs


class WeightedKmeansSelection(KmeansScoreSelection):
    """KmeansSelection's rows, weighted in proportion to their scores
    (utils.py:1381-1416, with the repairs of the module docstring)."""

    def __init__(self, train_dataset, num_pseudo, nc, seed, forgetting_flag=False,
                 score_type="entropy", embedding_flag=False, dist="euclidean"):
        super().__init__(train_dataset, num_pseudo, nc, seed, forgetting_flag, score_type,
                         embedding_flag, dist)

    def select(self):
        self.kmeans_cluster = _run_kmeans(self)
        return self.kmeans_cluster.get_arbitrary_pts(total_pts=self.num_pseudo)

    def get_weighted_subset(self, wt_vec=None):
        if len(self.core_idc) == 0:
            self.core_idc = self.select()
        n_coreset, n_train = len(self.core_idc), len(self.train_dataset)
        wt_vec_init = torch.as_tensor(self._get_uncertainty_score())[self.core_idc]
        self.wt_vec = (n_train / wt_vec_init.sum()) * wt_vec_init
        self.chosen_dataset = WeightedSubset(dataset=self.train_dataset, indices=self.core_idc,
                                             weights=self.wt_vec)
        return self.chosen_dataset


class ScoreCalculator:
    def __init__(self, outputs_prob, target, nc=10):
        self.outputs_prob = outputs_prob
        self.target = target
        self.nc = nc

    def least_confidence_score(self):
        return 1.0 - self.outputs_prob.max(1).values

    def entropy_score(self):
        return -self.outputs_prob.mul(torch.log(self.outputs_prob + 1e-20)).sum(1)

    def el2n_score(self):
        targets_onehot = F.one_hot(self.target.long(), num_classes=self.nc)
        return torch.linalg.vector_norm(x=(self.outputs_prob - targets_onehot), ord=2, dim=1)


class CoresetSelect:
    def __init__(self, train_dataset=None, test_dataset=None, data_minibatch=128, num_pseudo=100,
                 nc=2, architecture="logistic_regression", D=None, n_hidden=100, mc_samples=4,
                 init_sd=None, lr0net=1e-3, log_every=10, distr_fn=categorical_fn, seed=0,
                 score_method="kmeans", pretrain_epochs=5, data_folder=None,
                 load_from_saved=False, dnm=None, distance_fn="euclidean", last_layer_only=False,
                 multiple_pts_per_cluster=True, loaded_from_psvi=True, alpha_dirichlet=0,
                 choose_difficult=True, eps_source=None, clustering=None):
        if clustering not in (None, "hip"):
            raise ValueError(f'clustering is None or "hip" (got {clustering!r})')
        self.clustering = clustering
        self.architecture, self.score_method = architecture, score_method
        self.train_dataset, self.test_dataset = train_dataset, test_dataset
        self.num_pseudo, self.seed, self.nc, self.D, self.n_hidden = num_pseudo, seed, nc, D, n_hidden
        self.distr_fn, self.mc_samples, self.init_sd = distr_fn, mc_samples, init_sd
        self.data_minibatch, self.pretrain_epochs, self.lr0net = data_minibatch, pretrain_epochs, lr0net
        self.data_folder, self.load_from_saved, self.dnm = data_folder, load_from_saved, dnm
        self.distance_fn, self.last_layer_only = distance_fn, last_layer_only
        self.multiple_pts_per_cluster = multiple_pts_per_cluster
        self.loaded_from_psvi = loaded_from_psvi
        self.alpha_dirichlet, self.choose_difficult = alpha_dirichlet, choose_difficult
        self.eps_source = eps_source

    def select_data(self):
        _refuse_net(self.architecture)
        common = dict(train_dataset=self.train_dataset, num_pseudo=self.num_pseudo, nc=self.nc,
                      seed=self.seed)
        if self.score_method in _NO_KMEANS and not (self.clustering == "hip"
                                                    and self.score_method in _HIP_KMEANS):
            raise NotImplementedError(
                f"score_method {self.score_method!r} needs k-means clustering (sklearn / faiss) "
                "or the submodular package, which are not on the HIP path")
        kmeans_args = dict(embedding_flag=False, dist=self.distance_fn)
        if self.score_method == "kmeans":
            select_method = KmeansSelection(**common, **kmeans_args, data_folder=self.data_folder,
                                            dnm=self.dnm, multiple_pts=self.multiple_pts_per_cluster,
                                            loaded=self.loaded_from_psvi)
        elif self.score_method.startswith("scored_kmeans_"):
            select_method = KmeansScoreSelection(
                **common, **kmeans_args, score_type=self.score_method[14:],
                data_folder=self.data_folder, dnm=self.dnm,
                multiple_pts=self.multiple_pts_per_cluster, loaded=self.loaded_from_psvi,
                alpha=self.alpha_dirichlet, choose_difficult=self.choose_difficult)
        elif self.score_method == "weighted_kmeans":
            select_method = WeightedKmeansSelection(**common, **kmeans_args, score_type="entropy")
        elif self.score_method == "random":
            select_method = RandomSelection(**common)
        elif self.score_method in ["el2n", "least_confidence", "entropy", "forgetting"]:
            select_method = ScoreSelection(**common, score_type=self.score_method,
                                           data_folder=self.data_folder, dnm=self.dnm,
                                           loaded=self.loaded_from_psvi)
        elif re.fullmatch(r"scored_random_(el2n|forgetting|entropy|least_confidence)",
                          self.score_method):
            select_method = RandomScoreSelection(**common, score_type=self.score_method[14:])
        else:
            raise ValueError(f"{self.score_method} is not implemented")
        select_method.eps_source = self.eps_source
        select_method.pretrain(
            test_dataset=self.test_dataset, architecture=self.architecture, D=self.D,
            n_hidden=self.n_hidden, distr_fn=self.distr_fn, mc_samples=self.mc_samples,
            init_sd=self.init_sd, data_minibatch=self.data_minibatch,
            pretrain_epochs=self.pretrain_epochs, lr0net=self.lr0net, log_every=10,
            data_folder=self.data_folder, load_from_saved=self.load_from_saved, dnm=self.dnm)
        self.chosen_dataset = select_method.get_weighted_subset()
        log_core_idcs = select_method.core_idc
        log_core_wts = select_method.wt_vec.detach().numpy().tolist()
        self.wt_index = {str(k): v for k, v in zip(log_core_idcs, log_core_wts)}
