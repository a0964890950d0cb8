"""The tape planners' arithmetic as csrc/api.hip wrote it out before csrc/tape_plan.h existed: three copies of "columns per pass" (rt_plan_tapes,
fc_plan_tapes, t16_plan_dwtape), fc32's choice between column blocks and time segments, and the free-convection ensemble's segment count.  A literal
transcription, statement for statement, in Python integers (the C code's size_t and int never overflow on the grids of tests/test_tape_plan.py); it is
what tests/test_tape_plan.py holds the header to, and it is never derived from the header."""


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
