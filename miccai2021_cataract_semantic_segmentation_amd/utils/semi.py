"""Data side of the pseudo-label workflow (utils/semi_utis.py:6-23 of the reference)."""
from torch.utils.data import Dataset


class BalancedConcatDataset(Dataset):
    """item i is one item of every member: tuple(d[i % len(d)] for d in datasets); the length is the longest member's, the shorter ones
    wrap around.  With (labelled, pseudo-labelled) members a batch of such items is half labelled, half pseudo-labelled frames."""

    def __init__(self, *datasets):
        self.datasets = datasets
        dataset_lengths = [len(d) for d in self.datasets]
        self.max_len = max(dataset_lengths)
        self.min_len = min(dataset_lengths)

    def __getitem__(self, i):
        return tuple(d[i % len(d)] for d in self.datasets)

    def __len__(self):
        return self.max_len
