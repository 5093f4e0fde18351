"""Tree search over archived env states, on the device (shipsim.SearchTree over a shipsim.StateArchive).

The env is deterministic given its action sequence, so a node of the tree is a state: node i is cell i of an archive
of max_nodes cells, and an edge is the scoping angle that led there. One `round` sends every env down the tree at
once (select), starts it from its node's state (archive load), lets the widening envs take one decision and stores
their new nodes, rolls every env out to the episode's end and backs the returns up — without a copy to the host."""
import torch

from ... import shipsim_abi as abi
from ...shipsim import SearchTree


class TreeSearch:
    """TreeSearch(env, max_nodes, max_children=16, widen=(1, 1), c_explore=1.0) over a BatchedMultiShipRLEnv with
    K = 1..4 obstacle ships: W = env.n_envs workers per round. A node has at most max_children children and takes a
    new one while their number is below sqrt(widen[0] / widen[1] * (visits + 1)); c_explore scales the exploration
    term of the score (include/shipsim.h: shipsim_tree_select). Resets the env and stores the root. An env with
    per-env weather is refused with one root: weather stays with the slot, so a node replayed in another slot would
    be another episode, and one tree stands for one weather.

    n_roots = R > 1 searches a forest (shipsim_tree_select_forest): R trees in the one node pool, sharing the archive
    and every call of a round. Root r, node r, is env r after env.reset(); root_workers (R int32, default the even
    split W // R + (r < W % R)) says how many of the W workers start at each root, the roots being served in id order
    until the W are used up (workers left over sit the round out: leaf -1, no step, skipped by the backup). Under
    per-env weather root r is the reset state of env r under env r's weather: one tree per weather. The archive
    then keeps each node's weather (env.archive(M, weather=True)) and every load carries it to the slot, on the
    device — so the weather of the slots >= R is overwritten by the first load, and a slot's weather from then on is
    that of the node it last played. Under uniform weather the R trees are independent searches of one problem
    (root-parallel search). node_root[i] is the root above node i."""

    def __init__(self, env, max_nodes, max_children=16, widen=(1, 1), c_explore=1.0, n_roots=1, root_workers=None):
        self.n_roots = int(n_roots)
        if not 1 <= self.n_roots <= env.n_envs:
            raise ValueError(f"TreeSearch: n_roots must be in 1..n_envs = {env.n_envs}, not {n_roots}")
        carries_weather = env.weather() is not None
        if carries_weather and self.n_roots == 1:
            raise ValueError("TreeSearch: the env has per-env weather; weather stays with the slot, so a node loaded "
                             "into another slot would not replay its episode")
        if not 1 <= env.n_obs_ships <= abi.MAX_OBS:
            raise ValueError(f"TreeSearch: 1..{abi.MAX_OBS} obstacle ships, not {env.n_obs_ships}")
        self.env, self.device = env, env.device
        self.n_envs, self.max_nodes = env.n_envs, int(max_nodes)
        self.max_depth = int(env.cfg.max_sampling_frequency)  # decisions per episode
        if not 1 <= self.max_depth <= abi.TREE_MAX_DEPTH:
            raise ValueError(f"TreeSearch: max_sampling_frequency must be in 1..{abi.TREE_MAX_DEPTH}")
        self.widen, self.c_explore = (int(widen[0]), int(widen[1])), float(c_explore)
        dev, M, N = self.device, self.max_nodes, self.n_envs
        R = self.n_roots
        if R > M:
            raise ValueError(f"TreeSearch: {R} roots do not fit {M} nodes")
        self.tree = SearchTree(M, max_children, N, n_roots=R, device=dev)
        self.archive = env.archive(M, weather=True) if carries_weather else env.archive(M)
        self.root_workers = None
        if root_workers is not None:
            self.root_workers = torch.as_tensor(root_workers, dtype=torch.int32, device=dev).contiguous().reshape(-1)
            if self.root_workers.numel() != R:
                raise ValueError(f"TreeSearch: {self.root_workers.numel()} entries of root_workers for {R} roots")
        # per node, carried beside the archive (row M takes the writes of workers without a new node):
        self.node_reward = torch.zeros(M + 1, dtype=torch.float64, device=dev)  # the rewards from the root to the node
        self.node_obs = torch.zeros((M + 1, 8), dtype=torch.float32, device=dev)  # what the policy sees there
        self.node_root = torch.zeros(M + 1, dtype=torch.int32, device=dev)  # the root above the node
        self._cell_env = torch.empty(M + 1, dtype=torch.int32, device=dev)
        self._envs = torch.arange(N, dtype=torch.int32, device=dev)
        self.rounds = 0
        obs = env.reset()
        self.node_obs[:R] = obs[:R]
        self.node_root[:R] = self._envs[:R]
        self._cell_env.fill_(-1)
        self._cell_env[:R] = self._envs[:R]  # cell r takes env r: the roots
        self.archive.store(self._cell_env[:M])

    def round(self, propose, rollout):
        """One round of W = n_envs simulations. propose(obs) and rollout(obs) map (n_envs, 8) float32 observations
        to (n_envs,) float32 scoping angles [rad]: the action of a new edge, and the default policy from there to the
        episode's end. Returns a dict of per-env device tensors: leaf, expand, node, value, terminal, root (the
        root above the leaf), and of the decisions the env took in this round (none for a worker at a terminal leaf)
        events, their bits ORed, and ticks, their sum."""
        env, tree, M, N = self.env, self.tree, self.max_nodes, self.n_envs
        if self.n_roots == 1:
            leaf, expand = tree.select(self.max_depth, self.widen, self.c_explore)
            at = leaf.long()
            playing = None
        else:
            leaf, expand = tree.select(self.max_depth, self.widen, self.c_explore, root_workers=self.root_workers)
            playing = leaf >= 0  # (a worker no root received has leaf -1: row M, no load, no step, no backup)
            at = torch.where(playing, leaf, M).long()
        self.archive.load(leaf)
        widening = expand != 0
        obs = self.node_obs[at]
        action = torch.as_tensor(propose(obs), dtype=torch.float32, device=self.device).reshape(-1)
        o, r, d, info = env.step(action, active=widening)
        events = torch.where(widening, info["events"], 0)
        ticks = torch.where(widening, info["ticks"], 0).long()
        node = tree.expand(action)
        made = widening & (node >= 0)
        # the new nodes' states and what is carried with them: cell node[w] takes env w
        to = torch.where(made, node, M).long()
        self._cell_env.fill_(-1)
        self._cell_env.scatter_(0, to, self._envs)
        self.archive.store(self._cell_env[:M])
        cum = self.node_reward[at] + torch.where(widening, r, 0.0)
        obs = torch.where(widening[:, None], o, obs)
        self.node_reward.scatter_(0, to, cum)
        self.node_obs.scatter_(0, to[:, None].expand(-1, 8), obs)
        root = self.node_root[at]
        self.node_root.scatter_(0, to, root)
        if playing is not None:
            root = torch.where(playing, root, -1)
        terminal = widening & d
        # the rollout: everyone who is not at the end of an episode, to its end
        if playing is None:
            depth = tree.depth[at] + widening.int()
            alive = ~terminal & ((tree.flags[at] & 1) == 0) & (depth < self.max_depth)
        else:
            in_tree = at.clamp(max=M - 1)
            depth = tree.depth[in_tree] + widening.int()
            alive = playing & ~terminal & ((tree.flags[in_tree] & 1) == 0) & (depth < self.max_depth)
        for _ in range(self.max_depth):
            a = torch.as_tensor(rollout(obs), dtype=torch.float32, device=self.device).reshape(-1)
            o, r, d, info = env.step(a, active=alive)
            events = events | torch.where(alive, info["events"], 0)
            ticks = ticks + torch.where(alive, info["ticks"], 0)
            cum = cum + torch.where(alive, r, 0.0)
            obs = torch.where(alive[:, None], o, obs)
            depth = depth + alive.int()
            alive = alive & ~d & (depth < self.max_depth)
        tree.backup(cum, node, terminal=terminal.to(torch.uint8))
        self.rounds += 1
        return dict(leaf=leaf, expand=expand, node=node, value=cum, terminal=terminal, events=events, ticks=ticks,
                    root=root)

    def best_path(self, root=0):
        """The most-visited action sequence from the root (ties to the earlier child): a list of scoping angles and
        the list of node ids it passes. Copies the tree's statistics to the host."""
        root = int(root)
        if not 0 <= root < self.n_roots:
            raise ValueError(f"TreeSearch: root must be in 0..{self.n_roots - 1}, not {root}")
        n = self.tree.n_nodes
        nc = self.tree.n_children[:n].cpu().tolist()
        child = self.tree.child[:n].cpu().tolist()
        visits = self.tree.visits[:n].cpu().tolist()
        action = self.tree.action[:n].cpu().tolist()
        v, actions, nodes = root, [], [root]
        while nc[v] > 0 and len(actions) <= abi.TREE_MAX_DEPTH:
            v = max(child[v][:nc[v]], key=lambda a: visits[a])
            actions.append(action[v])
            nodes.append(v)
        return actions, nodes
