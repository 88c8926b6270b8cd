"""ext/kmeans/pairwise.py of the reference as plain tensor operations: the dense [N, N', M] difference table.  `lloyd`
does not use it (rr_kmeans_steps never builds that table); it is here because scripts import it."""


def pairwise_distance(data1, data2=None, device=-1):
    """Squared euclidean distances of data1 [N,M] against data2 [N',M] (data1 itself by default) -> [N,N'] with
    `.squeeze()` applied, as the reference returns it.  device != -1 moves both operands there first."""
    if data2 is None:
        data2 = data1
    if device != -1:
        data1, data2 = data1.cuda(device), data2.cuda(device)
    diff = data1.unsqueeze(dim=1) - data2.unsqueeze(dim=0)
    return (diff ** 2.0).sum(dim=-1).squeeze()


def group_pairwise(X, groups, device=0, fun=lambda r, c: pairwise_distance(r, c).cpu()):
    """{(i, j): fun(X[groups[i]], X[groups[j]])} for every ordered pair of index groups."""
    out = {}
    for i, rows in enumerate(groups):
        for j, cols in enumerate(groups):
            R, C = X[rows], X[cols]
            if device != -1:
                R, C = R.cuda(device), C.cuda(device)
            out[(i, j)] = fun(R, C)
    return out
