"""The tape planners' arithmetic as csrc/api.hip wrote it out before csrc/tape_plan.h existed: three copies of "columns per pass" (rt_plan_tapes,
fc_plan_tapes, t16_plan_dwtape), fc32's choice between column blocks and time segments, and the free-convection ensemble's segment count.  A literal
transcription, statement for statement, in Python integers (the C code's size_t and int never overflow on the grids of tests/test_tape_plan.py); it is
what tests/test_tape_plan.py holds the header to, and it is never derived from the header.  The second half restates the decisions that api_grad.hip and
api_ensemble.hip still made between their environment reads and allocations (on or off, the optional tapes, the overrides, the refusals) when those
moved to the header too: written from that text, before the C++ moved."""


def rt_block(n32, fit):
    """rt_plan_tapes, one pass of its loop (0: not even 1,024 columns)."""
    block = 0
    if fit >= n32:
        block = n32
    elif fit >= 1024:
        nb = (n32 + fit - 1) // fit
        block = (((n32 + nb - 1) // nb) + 1023) // 1024 * 1024
        if block > fit:
            block = (fit // 1024) * 1024
    return block


def fc_block(n32, fit):
    """fc_plan_tapes, the column-block part."""
    block = 0
    if fit >= n32:
        block = n32
    elif fit >= 32:
        nb = (n32 + fit - 1) // fit
        block = ((n32 + nb - 1) // nb + 31) // 32 * 32
        if block >= 8192:
            block = (block + 8191) // 8192 * 8192
        while block > fit:
            block -= 8192 if block > 8192 else 32
    return block


def t16_block(n16, fit, CT=16):
    """t16_plan_dwtape."""
    block = 0
    if fit >= n16:
        block = n16
    elif fit >= CT:
        nb = (n16 + fit - 1) // fit
        block = ((n16 + nb - 1) // nb + CT - 1) // CT * CT
        if block >= 4096:
            block = (block + 4095) // 4096 * 4096
        while block > fit:
            block -= 4096 if block > 4096 else CT
    return block


def fc_block_seg(n32, n_iv, cw, per_col_iv, budget, n_params):
    """fc_plan_tapes up to the environment overrides: (block, seg, the branch taken)."""
    fit = budget // (per_col_iv * n_iv)
    block, seg = 0, n_iv
    branch = "whole"
    if fit >= n32:
        block = n32
    else:
        block = fc_block(n32, fit)
        branch = "blocks"
        if block < 16384:
            branch = "nothing"
            cols_iv = budget // per_col_iv // 32 * 32
            if cols_iv >= 32:
                block = min(n32, cols_iv)
                branch = "segments of all columns" if block == n32 else "segments of a block"
                if block < n32 and block >= 8192:
                    block = block // 8192 * 8192
                seg = min(n_iv, budget // (per_col_iv * block))

                def slab_bytes(sg):
                    nsg, nblk = (n_iv + sg - 1) // sg, (n32 + block - 1) // block
                    return ((n32 // cw) + nblk * 512) * nsg * (n_params + 8) * 4

                seg0 = seg
                while seg > 1 and per_col_iv * block * seg + slab_bytes(seg) > budget:
                    seg -= 1
                if per_col_iv * block * seg + slab_bytes(seg) > budget:
                    seg = 0
                if seg == 0:
                    branch = "nothing (slab)"
                elif seg < seg0:
                    branch += ", slab shrinks seg"
    return block, seg, branch


def fc_ens_seg(n32, n_iv, cw, Nz, per_col_iv, budget, n_params):
    """fc_ens_plan_tapes: save intervals per time segment on a model's share of the budget."""
    def rest_bytes(sg):
        nsg = (n_iv + sg - 1) // sg
        return ((n32 // cw) + 512) * nsg * (n_params + 8) * 4 + n32 * Nz * 4

    seg = n_iv
    while seg > 1 and per_col_iv * n32 * seg + rest_bytes(seg) > budget:
        seg -= 1
    return seg


# ---- the planners of api_grad.hip / api_ensemble.hip as they stood before their decisions moved to csrc/tape_plan.h ---------------------------------------
# Environment switches arrive parsed, as the C code reads them: a flag is None (unset), False (atoi == 0) or True; a forced block or segment count
# is None (unset) or the integer atoi gives.  Every function returns the branch it took last, by name.

def fc_per_col_iv(substeps, nst, row_floats, mask_words, cw, has_switch_tape, conv_tape_floats_per_record):
    """fc_plan_tapes / fc_ens_plan_tapes: bytes of tape per column and save interval."""
    return substeps * nst * (row_floats * 4 + mask_words * 4 // cw + (8 if has_switch_tape else 0) +
                             (conv_tape_floats_per_record // 16 * 4 if conv_tape_floats_per_record else 0))


def fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab_seg_floats):
    """tape_plan.h at the parent: what a model of a (conv) ensemble owns; cslab_seg_floats = 0: fc_ens_model_bytes."""
    nsg = (n_iv + seg - 1) // seg
    plain = per_col_iv * n32 * seg + ((n32 // cw) + 512) * nsg * (n_params + 8) * 4 + n32 * Nz * 4
    return plain + ((nsg * cslab_seg_floats + 2 * n_params + 8) * 4 if cslab_seg_floats else 0)


def fc_tapes(n32, n_iv, cw, Nz, n_params, per_col_iv, free_b, forced_block, forced_seg, ensemble=False, K=1, cslab_seg_floats=0):
    """fc_plan_tapes (ensemble=False) and fc_ens_plan_tapes (ensemble=True) up to their first allocation:
    (block, seg, refused, bytes per model of an ensemble or 0, branch)."""
    if not ensemble:
        margin = (3 << 30) + (n32 // cw * 8 + 4096) * (n_params + 8) * 4 + n32 * Nz * 4
        block, seg, _ = fc_block_seg(n32, n_iv, cw, per_col_iv, free_b - margin if free_b > margin else 0, n_params)
        branch = "single, unforced"
        if forced_block is not None and forced_block >= 32:
            block = min(n32, (forced_block // 32) * 32)
            branch = "forced block, FC_SEG set to no count"
            if forced_seg is None:
                seg = n_iv
                branch = "forced block alone"
        if forced_seg is not None and forced_seg >= 1:
            seg = min(n_iv, forced_seg)
            branch = "both forced" if branch.startswith("forced block") else "forced seg alone"
        if block < 32 or seg < 1:
            return block, seg, True, 0, "single refused"
        return block, seg, False, 0, branch
    budget = (free_b - (3 << 30) if free_b > (3 << 30) else 0) // K
    seg = n_iv
    while seg > 1 and fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab_seg_floats) > budget:
        seg -= 1
    branch = "conv ensemble" if cslab_seg_floats else "ensemble, unforced"
    if forced_seg is not None and forced_seg >= 1:
        seg = min(n_iv, forced_seg)
        branch = "ensemble, forced seg"
    need = fc_conv_ens_model_bytes(n32, n_iv, cw, Nz, per_col_iv, n_params, seg, cslab_seg_floats)
    if need > budget:
        return n32, seg, True, need, "ensemble refused"
    return n32, seg, False, need, branch


def t16_tapes(n16, ns, n_bias, ag_rows, adj_split, lds_adj, lds_adj_noA, lds_adj_ag, per_col, per_col_rich, budget, dwtape, ztape, split_rich,
              forced_block, CT=16):
    """t16_plan_dwtape up to its first allocation: (status, need_z, block, rich, branch).  status: "taped", "inreg" (the in-register path follows) or
    the refusal.  lds_*: bytes of the three adjoint variants, the model's floats included."""
    want = dwtape if dwtape is not None else True
    branch = None
    if not want:
        branch = "forced off"
    if want and CT * ns > 6 * 512:
        want = False
        branch = "tile state too large"
    need_z = False
    if want and not ag_rows and lds_adj > 160 * 1024:
        if not (ztape is False) and lds_adj_noA <= 160 * 1024 and n_bias <= 4 * 512:
            need_z = True
        else:
            want = False
            branch = "ZTAPE=0 defeats needs-Z" if ztape is False and lds_adj_noA <= 160 * 1024 and n_bias <= 4 * 512 else "off for LDS"
    if ag_rows:
        if not want:
            return "refused: rows in global, off", need_z, 0, False, "rows-in-global refused (forced off)"
        if n_bias > 4 * 1024 or lds_adj_ag > 160 * 1024:
            return "refused: rows in global, too large", need_z, 0, False, "rows-in-global refused (too large)"
    block = 0
    rich_possible = adj_split and not (ztape is False) and not (split_rich is False)
    want_rich = False
    if want:
        fit = budget // per_col
        block = t16_block(n16, fit, CT)
        branch = "whole problem" if block == n16 else "equal blocks"
        if forced_block is not None and forced_block >= CT:
            block = min(n16, (forced_block // CT) * CT)
            branch = "forced block"
        if block <= 0:
            want = False
            branch = None
        want_rich = want and rich_possible and (split_rich is True or block <= 128 * CT)
        if want and adj_split and not (ztape is False) and split_rich is False:
            branch = "rich forced off"
        if want_rich:
            branch = "rich automatic" if split_rich is None else "rich forced on"
        if want_rich and block * per_col_rich > budget:
            fit_rich = budget // per_col_rich // CT * CT
            if split_rich is True and fit_rich >= CT:
                block = min(block, fit_rich)
                branch = "rich forced shrinks the block"
            else:
                want_rich = False
                branch = "rich forced but not one tile fits, so dropped" if split_rich is True else "rich automatic dropped for budget"
    if not want:
        if ag_rows:
            return "refused: rows in global, no fit", need_z, 0, False, "nothing fits with rows in global, so refused"
        return "inreg", need_z, 0, False, branch or "nothing fits, so in-register"
    if need_z and branch in ("whole problem", "equal blocks"):
        branch = "needs Z"
    return "taped", need_z, block, want_rich, branch


def t16_ens_tapes(K, n_tiles, per_model_rich, per_model_plain, budget, split_rich):
    """ens_plan_tapes up to its first allocation: (rich, bytes per model, refused, branch)."""
    forced = split_rich is not None
    rich = split_rich if forced else K * n_tiles <= 128
    branch = ("rich forced on" if rich else "rich forced off") if forced else ("rich automatic" if rich else "plain")
    if rich and not forced and K * per_model_rich > budget:
        rich = False
        branch = "rich gives way"
    need = per_model_rich if rich else per_model_plain
    if K * need > budget:
        return rich, need, True, "refused"
    return rich, need, False, branch


def rt_tapes(n32, per_col_x, per_col_2, per_col_z, budget, want_z, forced_block):
    """rt_plan_tapes up to its first allocation: (block, ztape, branch); block = 0: refused."""
    branch = "want_z off on entry" if not want_z else None
    block = 0
    for _ in range(2):
        if block != 0:
            break
        per_col = per_col_x + per_col_2 + (per_col_z if want_z else 0)
        block = rt_block(n32, budget // per_col)
        if block == 0:
            if want_z:
                branch = "Z1 dropped to fit"
            want_z = False
    if block and want_z:
        branch = "whole with Z1" if block == n32 else "blocks with Z1"
    if block == 0:
        branch = "nothing fits"
    if forced_block is not None and forced_block >= 32:
        block = min(n32, (forced_block // 32) * 32)
        branch = "forced block"
    return block, want_z, branch
