// The two limits of the lexical teacher kernels (include/snx.h "lexical teacher scores"), shared by teacher_lex.hip and
// the host code of snx_teacher_forward_m3 in teacher.hip, which refuses what the kernels' entry points would refuse
// before its first launch.
#pragma once

constexpr int LEX_MAX_SEQLEN = 8192;   // tokens of one sequence: 64 KB of 64-bit sort keys in LDS
constexpr int LEX_MAX_UNUSED = 8;      // unused ids: they travel as a kernel argument
