/* base_code.h -- a character of the MSA to the index of its group within a column: a c g t in either case 0 .. 3, a gap
 * ('-' or '_') 4, anything else 5 = no group (MC:303-330, RR:336-359).  For C, for the C++ host side and for device code. */
#ifndef PWR_BASE_CODE_H
#define PWR_BASE_CODE_H

#ifdef __HIPCC__
__host__ __device__
#endif
static inline int base_code(unsigned char ch)
{
    switch (ch) {
    case 'a': case 'A': return 0;
    case 'c': case 'C': return 1;
    case 'g': case 'G': return 2;
    case 't': case 'T': return 3;
    case '-': case '_': return 4;
    default: return 5;
    }
}

#endif /* PWR_BASE_CODE_H */
