"""The search options of the self-play layer and the ONE place that says which of them combine.  Imports neither torch nor
numpy: train_alphazero.py asks for the verdict before it pays for either.  Every entry point calls `resolve` once with the
inputs it has, keeps the record and hands one of its two views on: `keywords()` to the next entry point, `tree_keywords()` to
a tree context.  The combinations are one ordered table, RULES; what is handed on is another, HANDED_ON.  A new option is one
field, one row in each table, its value check in `resolve`, and one keyword in each signature that takes it."""
from dataclasses import dataclass


class OptionConflict(ValueError):
    """A refused combination: `option` names the option that refuses, `conflicts` those it does not go with (none: out of range)."""

    def __init__(self, message, option, conflicts=()):
        super().__init__(message)
        self.option, self.conflicts = option, tuple(conflicts)


@dataclass(frozen=True)
class SearchOptions:
    """The resolved options.  None is in the reference; every default is its search and the engine's launches and games without it.

    leaves_per_step K > 1: every search is leaf-parallel (engine.BatchedMCTS leaves_per_step): K descents per game and step
    with virtual visits, their leaves evaluated in one launch of up to K rows per game, ceil(num_simulations / K) steps per
    move -- for runs with few concurrent games, where a step costs the same whatever it carries.  The move around the search is
    unchanged (pass handling, root noise, the example record, the draws): it reads the root, and the root holds num_simulations
    visits at any K.  The None defaults of the evaluation-reuse options then mean OFF and no book is built: the leaf-parallel
    selection (k_mcts_multi) looks nothing up -- no kept pass value, no evaluation cache, no book -- and the tree context
    refuses the combination at create.  Asking for one of them explicitly, for aliased boards or for reference_quirks together
    with K > 1 is refused.  It changes which moves a search picks.

    fast_simulations N with full_search_probability P < 1: playout-cap randomisation.  Every move draws one uniform per game
    from the game's own counter stream (yy_selfplay_draw_budgets: keyed by seed, global game index and ply, so not by slot,
    batch or rank; SelfPlayWorker: one np.random.random() from the global stream): with probability P the game searches
    num_simulations, else N, in the same lockstep search (per-game budgets on the device, include/yy_engine.h
    yy_mcts_set_sim_budgets; the host issues the steps of num_simulations and reads no draw).  Root noise, pi, the temperature
    rule, the move draw and the z labels are unchanged; only the moves searched in full are recorded as examples (their `ply`
    is the game's ply).  Off -- N None or P == 1 -- draws nothing.  N outside 1 .. num_simulations or P outside (0, 1] is
    refused.

    tree_reuse: after the move draw every game's tree is re-rooted at the move played (engine.BatchedMCTS.advance; -1 = keep
    nothing for the games that did not search or that ended; SelfPlayWorker: MCTS.reuse_tree, as the reference calls it at
    self_play.py:192), and the next search continues from that subtree and tops its root up to the move's budget --
    num_simulations, or the playout-cap draw.  The host issues the same steps; a game whose kept root already holds part of its
    budget asks for fewer evaluator rows.  A kept tree belongs to its slot: when the draining batch is packed (compact_tail)
    every tree is dropped once, so with tree_reuse a game's transcript depends on when that happens.  It changes which moves a
    search picks.  The re-rooting kernel works on copied boards and one descent per step (include/yy_engine.h,
    yy_mcts_advance): refused with leaves_per_step > 1 or aliased boards.

    free_running: the games play their moves on the device, inside the search step (csrc/yy_selfplay_move.hip; DESIGN.md
    section 3).  A game whose search is complete records its example, draws and plays its move, handles passes and sets up its
    next root in the same step -- or ends, hands its labelled examples to the run's example buffer and lets the run's next game
    start in its slot -- while the other games keep simulating; the host only replays captured steps and, every poll_steps
    steps (default: four unrolled graphs), enqueues an asynchronous copy of the run's counters, reading the PREVIOUS poll's
    record.  The games are the lockstep engine's bit for bit (same seed, same game indices: every draw is keyed by (seed, game
    index, ply) and the evaluator sees a game's rows one by one), given an evaluator whose row results do not depend on the
    batch; collect() returns them sorted by (game_id, ply).  Evaluation reuse, the opening book and playout cap work as in
    lockstep; compact_tail / row_tiers do not apply (slots do not move: the compacted evaluator pays for live rows only).  The
    move kernel plays copied boards, one descent per step, the per-game counter streams and a fresh root per move: refused
    with leaves_per_step > 1, aliased boards, reference_quirks, rng="numpy" and tree_reuse (follow-ups; yy_mcts_advance empties
    the tree of every game it is not told to keep: re-rooting inside the step needs a "leave alone" action first).

    evaluation_symmetry "random": every position is shown to the evaluator under a board symmetry drawn for it (the dihedral
    group of a square board, the two flips of another) and its policy row is mapped back; the value is used as is.  The draw
    is a pure function of (symmetry_seed, position) from the Philox streams (include/yy_engine.h, YY_FLAG_EVAL_SYMMETRY) --
    not of slot, game, ply, simulation, batch or rank -- so evaluation reuse, the opening book (built through the same map and
    tied to the seed), lockstep against free-running and every other option work as without it.  symmetry_seed None = the
    engine's seed.  It changes which moves a search picks, unless the evaluator is exactly equivariant.  The reference has no
    such option: refused with aliased boards, reference_quirks and rng="numpy", which exist for transcript parity with it.

    forced_playouts k > 0 (KataGo: 2): forced playouts with policy target pruning at the search root (Wu, "Accelerating Self-Play
    Learning in Go", section 3.2; include/yy_engine.h YY_FLAG_FORCED_PLAYOUTS).  At the root a child that
    has been visited is visited again, before any score is looked at, while N * N < k * P * S (P its stored, noised prior, S the
    visits of the root's children), so a child that noise or a low prior makes interesting is judged on more than a handful of
    visits; pi -- the recorded example, the distribution the move is drawn from, root_policy() -- is then computed from counts
    from which every visit is taken back that the search would not have spent on the child by its score alone, and a child
    left with one visit is left with none.  Root visit counts (root_counts) stay raw.  Fast and full searches of the playout
    cap alike (KataGo switches it off in fast searches: a follow-up).  It changes which moves a search picks.  The forcing
    test is part of the one-descent selection on copied boards, and the reference has no such option: refused with
    leaves_per_step > 1, aliased boards, reference_quirks and rng="numpy".

    fpu_reduction r > 0 (KataGo: 0.2) with fpu_reduction_root (None: r; KataGo: 0 at a noised root): first-play urgency reduction
    in the PUCT selection (include/yy_engine.h YY_FLAG_FPU_REDUCTION).  The reference scores a child that
    has not been visited with q = 0, which is optimistic where the side to move is losing and pessimistic where it is winning.
    With the option such a child is scored with the mean value of its visited siblings less r * sqrt(the visited siblings' share
    of the prior): q_fpu = f32(f32(SW / SN) - f32(r * f32(sqrt(SP)))), the sums in fixed point so that they do not depend on the
    order of the children; q = 0 as before while no sibling is visited.  The root uses fpu_reduction_root (0: the siblings' mean
    itself), every node below it fpu_reduction.  Visited children, the exploration term, forced playouts and the pruned policy
    target are untouched.  It is a playing-strength parameter, so the arena and the evaluation matches take it as well as
    self-play; it goes with every leaves_per_step, both board semantics, the playout cap, tree reuse, free-running, evaluation
    symmetry, forced playouts, evaluation reuse and the book (which hold evaluator outputs only).  It changes which moves a
    search picks.  The reference has no such option: refused with reference_quirks and rng="numpy", which exist for transcript
    parity with it.

    shared_evaluations (True: SHARED_EVALUATIONS_DEFAULT_SLOTS slots, or a slot count, rounded up to a power of two; resolved
    to the slot count, 0: off): a shared evaluation table per tree context (engine.SharedEvaluations; include/yy_engine.h
    yy_mcts_set_shared_evaluations).  The per-game evaluation cache serves a position twice only inside the
    game that asked for it, and the opening book shares between games only what was enumerated before play.  With the option
    every fresh evaluator row also goes into a table of the context, and a leaf whose position ANY game of the context had
    evaluated in an earlier launch takes its row from there: no build phase, no stone limit, every board the tree kernels
    cover, memory for visited positions only (insert-only; a full probe window drops the insert).  The games played are the
    same, move for move; the evaluator sees fewer rows.  The default size costs at 8x8 what the 8-stone book costs (2.3 GB per
    context): a starting point, not a measured optimum.  Like evaluation_reuse="auto" it needs an evaluator that declares
    `row_independent` (ValueError otherwise, where the evaluator is known), copied boards and one descent per step: refused
    with board_semantics="aliased", leaves_per_step > 1 and reference_quirks.  It goes with evaluation reuse on or off, the
    book, the playout cap, tree reuse, free-running, evaluation symmetry (the table is tied to (mode, seed) like the book),
    forced playouts and fpu_reduction.  Every lane of SelfPlayLanes has a table of its own.

    shared_evaluations_replace (needs shared_evaluations; default False): the table in its replacing form
    (engine.SharedEvaluations(replace=True); include/yy_engine.h yy_mcts_set_shared_evaluations_replacing).
    Of all games that insert one position in one launch exactly one takes a slot, so the table fills with distinct positions
    only, and a sweep between tree steps -- once per move in lockstep, at every poll in free-running self-play -- evicts, once
    more than high_water of the slots are live, every entry that was neither inserted nor served since the last sweep that
    evicted (second chance over the whole table; SHARED_EVALUATIONS_HIGH_WATER): a table of a fixed size serves a run of any
    length.  The same games, move for move: a table only ever returns the evaluator's own row for a position, so no eviction
    or duplicate decision can change one.  Without shared_evaluations it is refused; with it, it is refused wherever
    shared_evaluations is.

    solver (default False): the MCTS-Solver (Winands et al. 2008; Lc0's "certainty propagation"; include/yy_engine.h
    YY_FLAG_SOLVER).  Yin-Yang games end by filling the board, so from the middle game on many descents run
    into terminal positions, whose exact results the reference only ever averages into its value sums.  With the option a node
    may be proven WIN, LOSS or DRAW for its side to move: a terminal node is; a node with children is a WIN when some child is a
    LOSS for the opponent, and a LOSS or DRAW once all its children exist and are proven.  A position whose mover has no move is
    never proven, so every proof consists of real moves and terminal positions only.  A descent that reaches a proven node below
    the root stops there, backs the exact value up and asks for no evaluator row; the root itself keeps being searched.
    Scores, visit counts, pi, the temperature rule and self-play's move draw are untouched: the option changes which descents
    are made, not how they are scored.  AlphaZeroPlayer and the arena play, at temperature 0, the most visited root child that
    is proven lost for the opponent when there is one.  It goes with the playout cap, tree reuse (statuses travel with the
    kept nodes), free-running, evaluation reuse, the book, the shared table, evaluation symmetry, forced playouts and
    fpu_reduction.  Proofs under virtual visits and on a board that changes under a node are follow-ups, and the reference has
    no such option: refused with leaves_per_step > 1, board_semantics="aliased", reference_quirks and rng="numpy".

    gumbel_root m in 2 .. 64 (the paper: 16) with gumbel_c_visit (None: 50) and gumbel_c_scale (None: 1.0): the Gumbel root search
    (Danihelka et al., ICLR 2022; include/yy_engine.h YY_FLAG_GUMBEL_ROOT).  Every root draws a Gumbel
    variable per action from the game's own counter stream, spends the search's budget -- num_simulations, or the playout-cap
    draw -- by sequential halving over the m actions of largest g + log P, records softmax(log P + sigma(completed q)) as pi
    and plays the most visited child of largest g + log P + sigma(q) at every ply: the temperature rule and the move draw are
    not consulted.  Below the root the search is unchanged.  dirichlet_epsilon = 0 is recommended with it.  It goes with the
    playout cap, free-running, evaluation symmetry, evaluation reuse, the book, both shared tables and fpu_reduction (below the
    root only).  It changes which moves a search picks.  Sequential halving plans the visits of a fresh root in the one-descent
    selection, and the reference has no such option: refused with leaves_per_step > 1, board_semantics="aliased",
    reference_quirks, rng="numpy", forced_playouts, tree_reuse and solver (each a follow-up).

    gumbel_interior (needs gumbel_root; default False): the rest of Gumbel AlphaZero (the paper's section 5 and appendix D;
    include/yy_engine.h YY_FLAG_GUMBEL_INTERIOR).  The root keeps its own network value, an unvisited child
    is completed with v_mix -- that value mixed with the prior-weighted mean of the visited children's -- in the policy target,
    and a descent below the root visits the child of largest pi'(a) - N(a) / (1 + sum N), pi' the same completed-Q improved
    policy, instead of the PUCT choice: deterministic, no exploration constant, no first-play urgency.  The arithmetic is
    reproducible bit for bit (no log, an exponential of the project's own, integer sums).  It goes with whatever gumbel_root
    goes with and is refused wherever gumbel_root is; fpu_reduction has nothing left to act on and is refused with it.  It
    changes which moves a search picks."""
    leaves_per_step: int = 1
    fast_simulations: int = None            # None: the playout cap is off; full_search_probability is then 1.0
    full_search_probability: float = 1.0
    tree_reuse: bool = False
    free_running: bool = False
    evaluation_symmetry: str = "off"
    symmetry_seed: int = None               # None: the engine's seed
    forced_playouts: float = 0.0            # 0.0: off
    fpu_reduction: float = 0.0              # 0.0: off
    fpu_reduction_root: float = 0.0         # resolved: fpu_reduction where it was not given; 0.0 when the option is off
    shared_evaluations: int = 0             # slots of the shared evaluation table (a power of two); 0: off
    shared_evaluations_replace: bool = False  # the table deduplicates inserts and evicts (needs shared_evaluations)
    solver: bool = False                    # proven wins, losses and draws in the tree
    gumbel_root: int = 0                    # m of the Gumbel root search; 0: off
    gumbel_c_visit: float = 0.0             # resolved: 50 where it was not given; 0.0 when the option is off
    gumbel_c_scale: float = 0.0             # resolved: 1.0 where it was not given; 0.0 when the option is off
    gumbel_interior: bool = False           # v_mix and completed-Q selection below the root (needs gumbel_root)

    @property
    def playout_cap(self):
        """The two playout-cap keywords, {} when it is off."""
        return {} if self.fast_simulations is None else dict(fast_simulations=self.fast_simulations,
                                                              full_search_probability=self.full_search_probability)

    def _handed(self, tree_only=False):
        return dict(leaves_per_step=self.leaves_per_step,
                    **{f: getattr(self, f) for switch, fields, tree in HANDED_ON for f in fields
                       if getattr(self, switch) != getattr(SearchOptions, switch) and (tree or not tree_only)})

    def keywords(self):
        """The keywords to hand to the next layer: leaves_per_step always, the groups of HANDED_ON that are on."""
        return self._handed()

    def tree_keywords(self, seed=None):
        """The keywords of keywords() that a tree context (engine.BatchedMCTS) takes; `seed` stands in for a symmetry_seed of
        None."""
        kw = self._handed(tree_only=True)
        if "symmetry_seed" in kw and kw["symmetry_seed"] is None:
            kw["symmetry_seed"] = seed
        return kw


# What a record hands on beside leaves_per_step, as groups: (the field that switches the group on -- it is on when the field
# is not at its default --, the fields handed on then, whether a tree context takes them).  Both views read this table.
HANDED_ON = (("fast_simulations", ("fast_simulations", "full_search_probability"), False),
             ("tree_reuse", ("tree_reuse",), False),
             ("free_running", ("free_running",), False),
             ("evaluation_symmetry", ("evaluation_symmetry", "symmetry_seed"), True),
             ("forced_playouts", ("forced_playouts",), True),
             ("fpu_reduction", ("fpu_reduction", "fpu_reduction_root"), True),
             ("shared_evaluations", ("shared_evaluations",), False),
             ("shared_evaluations_replace", ("shared_evaluations_replace",), False),
             ("solver", ("solver",), True),
             ("gumbel_root", ("gumbel_root", "gumbel_c_visit", "gumbel_c_scale"), True),
             # a sub-option of the Gumbel group, in a row of its own so that both views carry it only when it is on
             ("gumbel_interior", ("gumbel_interior",), True))


def forced_k(forced_playouts):
    """forced_playouts as the device takes it: 0.0 for None / 0 (off), else the positive finite float.  OptionConflict for
    anything else."""
    if forced_playouts is None:
        return 0.0
    try:
        k = float(forced_playouts)
    except (TypeError, ValueError):
        k = -1.0
    if not 0.0 <= k < float("inf"):
        raise OptionConflict(f"forced_playouts={forced_playouts!r}: a finite number >= 0 (0 / None: off; KataGo uses 2)", "forced_playouts")
    return k


GUMBEL_C_VISIT, GUMBEL_C_SCALE = 50.0, 1.0   # the paper's board-game values


def gumbel_m(gumbel_root, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False):
    """(m, c_visit, c_scale) as the device takes them: (0, 0.0, 0.0) for gumbel_root None / 0 (off), else the int m in 2 .. 64,
    the finite c_visit >= 0 (None: 50) and the finite c_scale > 0 (None: 1.0).  OptionConflict naming gumbel_root for anything
    else, a c value or gumbel_interior (None / False / True) without the option included."""
    def num(x):
        try:
            return float(x)
        except (TypeError, ValueError):
            return float("nan")

    if gumbel_interior not in (None, False, True):
        raise OptionConflict(f"gumbel_interior={gumbel_interior!r}: True or False", "gumbel_root")
    if gumbel_root is None or gumbel_root is False or (not isinstance(gumbel_root, bool) and gumbel_root == 0):
        if gumbel_interior:
            raise OptionConflict("gumbel_interior=True without gumbel_root: it completes the Gumbel root search below the root, "
                                 "and gumbel_root 0 / None switches that off", "gumbel_root")
        if gumbel_c_visit is not None or gumbel_c_scale is not None:
            raise OptionConflict("gumbel_c_visit / gumbel_c_scale without gumbel_root: they belong to the option, and gumbel_root "
                                 "0 / None switches it off", "gumbel_root")
        return 0, 0.0, 0.0
    try:
        m = int(gumbel_root)
        if m != gumbel_root or isinstance(gumbel_root, bool):
            m = -1
    except (TypeError, ValueError):
        m = -1
    if not 2 <= m <= 64:
        raise OptionConflict(f"gumbel_root={gumbel_root!r}: the number of root actions sequential halving starts from, an int in "
                             "2 .. 64 (0 / None: off; the paper uses 16)", "gumbel_root")
    cv = GUMBEL_C_VISIT if gumbel_c_visit is None else num(gumbel_c_visit)
    if not 0.0 <= cv < float("inf"):
        raise OptionConflict(f"gumbel_c_visit={gumbel_c_visit!r}: a finite number >= 0 (None: 50)", "gumbel_root")
    cs = GUMBEL_C_SCALE if gumbel_c_scale is None else num(gumbel_c_scale)
    if not 0.0 < cs < float("inf"):
        raise OptionConflict(f"gumbel_c_scale={gumbel_c_scale!r}: a finite number > 0 (None: 1.0)", "gumbel_root")
    return m, cv, cs


SHARED_EVALUATIONS_DEFAULT_SLOTS = 1 << 23   # 8x8: 280 bytes a slot = 2.3 GB, the 8-stone opening book's size
# replacing table: the share of live slots above which a sweep evicts.  profiles/shared_evaluations_replace.json holds the
# comparison of 0.5, 0.75 and 0.9 (tools/shared_evaluations.py --high-water)
SHARED_EVALUATIONS_HIGH_WATER = 0.75


def shared_slots(shared_evaluations):
    """shared_evaluations as the device takes it: 0 for None / False (off), SHARED_EVALUATIONS_DEFAULT_SLOTS for True, an int
    slot count rounded up to a power of two (at least 64, at most 2^30).  OptionConflict for anything else."""
    if shared_evaluations is None or shared_evaluations is False:
        return 0
    if shared_evaluations is True:
        return SHARED_EVALUATIONS_DEFAULT_SLOTS
    try:
        n = int(shared_evaluations)
        if n != shared_evaluations:
            n = -1
    except (TypeError, ValueError):
        n = -1
    if not 0 < n <= 1 << 30:
        raise OptionConflict(f"shared_evaluations={shared_evaluations!r}: None / False (off), True (the default size) or a slot "
                             "count in 1 .. 2^30", "shared_evaluations")
    slots = 64
    while slots < n:
        slots *= 2
    return slots


def fpu_r(fpu_reduction, fpu_reduction_root=None):
    """(r, r_root) as the device takes them: (0.0, 0.0) for fpu_reduction None / 0 (off), else the positive finite r and the
    root's finite r_root >= 0 (None: r).  OptionConflict naming fpu_reduction for anything else, a root value without the option
    included."""
    def num(x):
        try:
            return float(x)
        except (TypeError, ValueError):
            return -1.0

    r = 0.0 if fpu_reduction is None else num(fpu_reduction)
    if not 0.0 <= r < float("inf"):
        raise OptionConflict(f"fpu_reduction={fpu_reduction!r}: a finite number >= 0 (0 / None: off; KataGo uses 0.2)", "fpu_reduction")
    root = (r if fpu_reduction_root is None else num(fpu_reduction_root))
    if not 0.0 <= root < float("inf"):
        raise OptionConflict(f"fpu_reduction_root={fpu_reduction_root!r}: a finite number >= 0 (None: fpu_reduction; KataGo uses 0 "
                             "at a noised root)", "fpu_reduction")
    if not r and root:
        raise OptionConflict(f"fpu_reduction_root={fpu_reduction_root!r} without fpu_reduction: the root's value belongs to the "
                             "option, and fpu_reduction 0 / None switches it off", "fpu_reduction")
    return r, root


# The conflict rules, in the ONE order they are asked in: (the option that refuses, the inputs it does not go with -- named in
# this order --, why).  Two broken rules name the earlier one everywhere.  Every option's value check comes right before its
# first rule, the playout cap's range checks between tree_reuse and leaves_per_step (resolve).
_NO_SUCH_OPTION = "the reference has no such option, so it does not go with what exists for transcript parity with it -- not with"
RULES = (
    ("evaluation_symmetry", ("board_semantics", "reference_quirks", "rng"), _NO_SUCH_OPTION),
    ("forced_playouts", ("leaves_per_step", "board_semantics", "reference_quirks", "rng"),
     "the forcing test is part of the one-descent selection on copied boards, and the reference has no such option -- not with"),
    ("gumbel_root", ("leaves_per_step", "board_semantics", "reference_quirks", "rng", "forced_playouts", "tree_reuse", "solver"),
     "sequential halving plans the visits of a fresh root in the one-descent selection on copied boards, its draws are the "
     "device's counter streams, and the reference has no such option -- not with"),
    ("gumbel_root", ("fpu_reduction",),
     "gumbel_interior=True selects below the root by the improved policy, so no PUCT score is left for first-play urgency to act "
     "on -- not with"),
    ("free_running", ("leaves_per_step", "board_semantics", "reference_quirks", "rng", "tree_reuse"),
     "the in-step move plays copied boards with one descent per step, the device's counter streams and a fresh root per move "
     "-- not with"),
    ("tree_reuse", ("leaves_per_step",), "the tree is re-rooted for one descent per step only -- not with"),
    ("tree_reuse", ("board_semantics",), "a kept subtree needs every node's own board -- not with"),
    ("leaves_per_step", ("board_semantics", "reference_quirks", "evaluation_reuse", "opening_book"),
     "a leaf-parallel search runs on copied boards, evaluates every leaf and has no book -- not with"),
    ("fpu_reduction", ("reference_quirks", "rng"), _NO_SUCH_OPTION),
    ("shared_evaluations", ("board_semantics", "leaves_per_step", "reference_quirks"),
     "a shared evaluation table serves a position's stored row to every game, which needs copied boards, one descent per step "
     "and a search that is not the reference's literal one -- not with"),
    ("shared_evaluations_replace", ("shared_evaluations",),
     "it is the replacing form of the shared evaluation table -- not without"),
    ("solver", ("leaves_per_step", "board_semantics", "reference_quirks", "rng"),
     "a proof belongs to a node whose position does not change and to one descent per step, and the reference has no such "
     "option -- not with"))


def _ask(option, rendered, given):
    """The rules of `option`, which is on and renders as `rendered`: OptionConflict for the first of them that `given` -- input
    -> (it is in the way, as a message renders it) -- breaks."""
    for _, others, why in (r for r in RULES if r[0] == option):
        bad = [n for n in others if given[n][0]]
        if bad:
            raise OptionConflict(f"{rendered}: {why} {', '.join(given[n][1] for n in bad)}", option, bad)


def resolve(num_simulations=None, leaves_per_step=1, board_semantics="copied", reference_quirks=False, rng="philox",
            evaluation_reuse=(), opening_book=None, fast_simulations=None, full_search_probability=1.0, tree_reuse=False,
            free_running=False, evaluation_symmetry="off", symmetry_seed=None, forced_playouts=None,
            fpu_reduction=None, fpu_reduction_root=None, shared_evaluations=None, shared_evaluations_replace=False,
            solver=False, gumbel_root=None, gumbel_c_visit=None, gumbel_c_scale=None, gumbel_interior=False):
    """The SearchOptions of one combination, or OptionConflict (a ValueError) -- on the host, before anything touches the
    device.  Every default means "off" / "not given", so a caller passes what it has.  evaluation_reuse: the reuse options as
    given (None = the default, which K > 1 resolves to off); opening_book: an engine.OpeningBook or a stone count (None and
    counts <= 0: no book); num_simulations None: no upper bound for fast_simulations.  The rules are asked in the one fixed
    order of RULES, so two broken rules name the same option everywhere.  forced_playouts, fpu_reduction: None and 0 = off;
    shared_evaluations: None and False = off; shared_evaluations_replace: None and False = off."""
    K = max(1, int(leaves_per_step))
    given = dict(leaves_per_step=(K > 1, f"leaves_per_step={leaves_per_step}"),
                 board_semantics=(board_semantics == "aliased", 'board_semantics="aliased"'),
                 reference_quirks=(reference_quirks, "reference_quirks=True"), rng=(rng != "philox", f'rng="{rng}"'),
                 tree_reuse=(tree_reuse, "tree_reuse=True"), solver=(solver, "solver=True"),
                 evaluation_reuse=(any(x is not None and bool(x) for x in evaluation_reuse),
                                   "evaluation reuse (reuse_pass_value / reuse_transpositions / keep_evaluations / evaluation_reuse)"),
                 opening_book=(opening_book is not None and not (isinstance(opening_book, int) and opening_book <= 0),
                               "an opening book"))
    if evaluation_symmetry not in ("off", "random"):
        raise OptionConflict(f'evaluation_symmetry={evaluation_symmetry!r}: "off" or "random"', "evaluation_symmetry")
    sym = evaluation_symmetry != "off"
    if sym:
        _ask("evaluation_symmetry", f'evaluation_symmetry="{evaluation_symmetry}"', given)
    forced = forced_k(forced_playouts)
    given["forced_playouts"] = (forced, f"forced_playouts={forced_playouts}")
    if forced:
        _ask("forced_playouts", given["forced_playouts"][1], given)
    gm, gcv, gcs = gumbel_m(gumbel_root, gumbel_c_visit, gumbel_c_scale, gumbel_interior)
    # first-play urgency is in the way of the Gumbel group only when gumbel_interior is on (its value is checked below)
    given["fpu_reduction"] = (bool(gumbel_interior) and fpu_reduction is not None and fpu_reduction != 0,
                              f"fpu_reduction={fpu_reduction}")
    if gm:
        _ask("gumbel_root", f"gumbel_root={gumbel_root}", given)
    if free_running:
        _ask("free_running", "free_running=True", given)
    if tree_reuse:
        _ask("tree_reuse", "tree_reuse=True", given)
    P = float(full_search_probability)
    if not 0.0 < P <= 1.0:
        raise OptionConflict(f"full_search_probability={full_search_probability}: the share of full searches lies in (0, 1]",
                             "full_search_probability")
    fast = None if fast_simulations is None else int(fast_simulations)
    if fast is not None and fast < 1:
        raise OptionConflict(f"fast_simulations={fast_simulations}: a fast search runs at least 1 simulation", "fast_simulations")
    if fast is not None and num_simulations is not None and fast > int(num_simulations):
        raise OptionConflict(f"fast_simulations={fast_simulations}: a fast search runs no more than num_simulations={num_simulations}",
                             "fast_simulations", ["num_simulations"])
    if K > 1:
        _ask("leaves_per_step", f"leaves_per_step={K}", given)
    fpu, fpu_root = fpu_r(fpu_reduction, fpu_reduction_root)
    if fpu:
        _ask("fpu_reduction", f"fpu_reduction={fpu_reduction}", given)
    shared = shared_slots(shared_evaluations)
    given["shared_evaluations"] = (not shared, "shared_evaluations")       # in the way of its replacing form when it is off
    if shared:
        _ask("shared_evaluations", f"shared_evaluations={shared_evaluations}", given)
    if shared_evaluations_replace not in (None, False, True):
        raise OptionConflict(f"shared_evaluations_replace={shared_evaluations_replace!r}: True or False", "shared_evaluations_replace")
    if shared_evaluations_replace:
        _ask("shared_evaluations_replace", "shared_evaluations_replace=True", given)
    if solver not in (None, False, True):
        raise OptionConflict(f"solver={solver!r}: True or False", "solver")
    if solver:
        _ask("solver", "solver=True", given)
    cap = fast is not None and P < 1.0
    return SearchOptions(K, fast if cap else None, P if cap else 1.0, bool(tree_reuse), bool(free_running),
                         evaluation_symmetry, None if not sym or symmetry_seed is None else int(symmetry_seed), forced, fpu, fpu_root,
                         shared, bool(shared_evaluations_replace), bool(solver), gm, gcv, gcs, bool(gumbel_interior))
