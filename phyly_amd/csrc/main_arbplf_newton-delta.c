/* arbplf-newton-delta: JSON on stdin -> JSON on stdout, exit status 0 on success.
 * Drop-in for the reference's src/arbplf-newton-delta.c (run_json_script with newton_delta_query). */
#include "arbplf.h"

int main(void)
{
    return arbplf_run_stdin(arbplf_newton_delta_string);
}
