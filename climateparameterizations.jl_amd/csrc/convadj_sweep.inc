// convadj_sweep.inc — one convective_adjustment!(model, Δt, K) step of ONE column (free_convection/src/oceananigans_nn.jl:13-40,
// free_convection/double_gyre_nn.jl:27-62): the switch pattern and the Thomas sweep, included as TEXT by convadj_kernel (column_ops.hip) and by
// the free-convection embedded step (engine_fc_embed.hip).  Text rather than a function, so that the code the compiler sees in convadj_kernel is
// what it was before the sweep was shared.  In scope: NZ; float* t, the column's NZ levels, solved in place (k = 0 deepest; an LDS row in both
// callers); const float* halo_bottom, halo_top, arrays of halo cells or null, and ca_i, the column's index in them; float c = Δt/Δz², K.
        float x[NZ], cp[NZ];
#pragma unroll
        for (int k = 0; k < NZ; k++) x[k] = t[k];
        const float ck = c * K;
        // κ of cell k as c·κ_k: statically unstable where T[k+1] - T[k-1] < 0; the halo cells are the caller's (they carry
        // the field's boundary conditions) or, absent, the nearest interior value (zero-gradient fill)
        const float below = halo_bottom ? halo_bottom[ca_i] : x[0];
        const float above = halo_top ? halo_top[ca_i] : x[NZ - 1];
        float kk[NZ];
#pragma unroll
        for (int k = 0; k < NZ; k++) kk[k] = ((k + 1 < NZ ? x[k + 1] : above) - (k > 0 ? x[k - 1] : below)) < 0.0f ? ck : 0.0f;
        // forward elimination
        float inv = 1.0f / (1.0f + kk[0] + kk[1]);
        cp[0] = -kk[1] * inv;
        x[0] = x[0] * inv;
#pragma unroll
        for (int k = 1; k < NZ; k++) {
            const float a = -kk[k];
            const float b = 1.0f + kk[k] + (k < NZ - 1 ? kk[k + 1] : 0.0f);
            inv = 1.0f / (b - a * cp[k - 1]);
            cp[k] = (k < NZ - 1 ? -kk[k + 1] : 0.0f) * inv;
            x[k] = (x[k] - a * x[k - 1]) * inv;
        }
        // back substitution
#pragma unroll
        for (int k = NZ - 2; k >= 0; k--) x[k] -= cp[k] * x[k + 1];
#pragma unroll
        for (int k = 0; k < NZ; k++) t[k] = x[k];
