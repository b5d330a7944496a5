"""Host model of a DeviceIndex: {tenant: {id: row}}, plain Python and numpy.

What a long-lived shard must hold after any sequence of upserts and deletes is stated here once, with no row order in
it: the expected answers of the lifecycle tests are the project's references (oracle.hamming_topk, cosine_ref.CosineRef)
run over `arrays(tenant)`, and neither depends on where a row sits.

Beside the model proper, `device_order(tenant)` replays the index's placement rule (a new id takes the next row, a delete
moves the last row into the hole).  It only AIMS operations -- "delete the last row", "delete the row the previous
delete moved" -- and never enters an expected answer: were it wrong, a scenario would miss the branch it names, not
pass a wrong result."""
import numpy as np


class IndexModel:
    def __init__(self, dtype, row_shape=()):
        self.dtype = np.dtype(dtype)
        self.row_shape = tuple(row_shape)
        self.tenants = {}        # tenant -> {id: row}
        self._order = {}         # tenant -> [id, ...]   (aiming aid, see above)
        self._at = {}            # tenant -> {id: position in _order}
        self._arrays = {}        # tenant -> cached arrays() result

    # ---- the model ----
    def upsert(self, tenant, ids, rows):
        """The last occurrence of an id inside one batch wins."""
        ids = [int(i) for i in np.asarray(ids, dtype=np.uint64).reshape(-1)]
        rows = np.asarray(rows, dtype=self.dtype).reshape((len(ids),) + self.row_shape)
        d = self.tenants.setdefault(tenant, {})
        order, at = self._order.setdefault(tenant, []), self._at.setdefault(tenant, {})
        last = {i: j for j, i in enumerate(ids)}
        for j, i in enumerate(ids):
            if last[i] != j:
                continue
            if i not in d:
                at[i] = len(order)
                order.append(i)
            d[i] = rows[j].copy()
        self._arrays.pop(tenant, None)

    def delete(self, tenant, ids):
        """-> rows removed: an unknown id counts nothing, a repeated id once (as ucfp_index_delete reports)."""
        d = self.tenants.get(tenant)
        if d is None:
            return 0
        removed = 0
        order, at = self._order[tenant], self._at[tenant]
        for i in (int(i) for i in np.asarray(ids, dtype=np.uint64).reshape(-1)):
            if i not in d:
                continue
            del d[i]
            removed += 1
            r, moved = at.pop(i), order.pop()
            if moved != i:
                order[r] = moved
                at[moved] = r
        self._arrays.pop(tenant, None)
        return removed

    def size(self, tenant):
        return len(self.tenants.get(tenant, ()))

    def arrays(self, tenant):
        """-> (ids u64 [n], rows [n, ...]) of a tenant, by ascending id (any order would do)."""
        if tenant not in self._arrays:
            d = self.tenants.get(tenant, {})
            ids = np.fromiter(d.keys(), dtype=np.uint64, count=len(d))
            rows = np.empty((len(d),) + self.row_shape, self.dtype)
            for j, r in enumerate(d.values()):
                rows[j] = r
            by_id = np.argsort(ids, kind="stable")
            self._arrays[tenant] = (ids[by_id], rows[by_id])
        return self._arrays[tenant]

    def row(self, tenant, i):
        return self.tenants[tenant][int(i)]

    # ---- aiming aid ----
    def device_order(self, tenant):
        """Ids in the row order the index's placement rule gives (read-only view)."""
        return self._order.get(tenant, [])
